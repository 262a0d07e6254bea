"""Shared by tests/test_rcan_cpu.py and tests/test_rcan_gpu.py: the reference fixture of the RCAN generator
(tests/golden/make_rcan_fixtures.py -> tests/golden/rcan_reference.npz) and the weights it was generated with."""
import argparse
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G = np.load(os.path.join(GOLDEN, "rcan_reference.npz"))
SEQ = np.load(os.path.join(GOLDEN, "colour_reference.npz"))          # the sequence the fixture was made from: `low`, `flow_filled`
PREMISE = 4e-5          # fp32 against fp64, single step, of the reference itself: the project's premise for its 1e-4 comparisons
BOUND = 1e-4            # the project's standing single-step tolerance against the reference
CASES = {"a": dict(cin=56, own=8, mask=[0, 1, 2], cout=3),
         "b": dict(cin=52, own=4, mask=[0, 1, 2], cout=3)}
LINEAR_GAIN = 6.0


def fill_state_dict(net, seed):
    """The rule of the generator (the weights are not stored): the same ``numpy.random.RandomState(seed)`` stream -- for every key in
    ``state_dict()`` order n = standard_normal(shape); a convolution weight [a, b, 3, 3] is ``gain * sqrt(2 / (9 b)) * n`` (He scale;
    gain 0.25 for every block's second convolution and the ``post`` layers of the groups and of ``net.rir``, 0.1 for ``net.post``, else
    1), a Linear weight [a, b] ``6 n / sqrt(b)``, ``net.post.bias`` ``0.5 + 0.05 n``, every other bias ``0.05 n``."""
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


def rcan_net(case):
    """The fixture's network of ``case``: the full 10 x 20, ``opt`` None as the reference's script passes it."""
    from isosurfacesuperresolution_amd import models
    c = CASES[case]
    return fill_state_dict(models.createNetwork('RCAN', 4, c["cin"], c["mask"], c["cout"], None).eval(), int(G["weight_seed"]))


def small_rcan(groups, blocks, cin=56, seed=5):
    """A small network of the same rule (``rcanGroups`` / ``rcanBlocks``)."""
    from isosurfacesuperresolution_amd import models
    opt = argparse.Namespace(rcanGroups=groups, rcanBlocks=blocks)
    return fill_state_dict(models.createNetwork('RCAN', 4, cin, [0, 1, 2], 3, opt).eval(), seed)
