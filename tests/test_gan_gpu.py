"""Adversarial training on the HIP path against the reference (tests/golden/gan_reference.npz): cases a, b and c of test_gan_cpu.py on the
device, with the same bars (gan_common.py).  During the adversarial step no layer may fall back to PyTorch's convolutions, and the
stride-2 layers' launches must be the stride-2 kernels' (csrc/sr_conv_stride2.hip)."""
import warnings

import pytest

import gan_common as C
from train_route_common import observed

pytestmark = pytest.mark.gpu


def test_discriminators_match_the_reference_on_the_device():
    _, families, names = observed(lambda: C.check_discriminators("cuda"))
    # two (small) or three (large) halvings' worth of stride-2 layers per network: 2 + 3 + 2 + 3
    assert names.count("conv3x3s2_fwd_kernel") == 10, names


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "module"])
def test_criterion_with_adversarial_terms_matches_the_reference_on_the_device(fused):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _, families, names = observed(lambda: C.check_criterion("cuda", fused=fused))
    assert not [str(c.message) for c in caught if issubclass(c.category, RuntimeWarning)], [str(c.message) for c in caught]
    # generator side: data gradients through all three discriminators, no weight gradient wanted ... then train_discriminator
    for kernel in ("conv3x3s2_fwd_kernel", "conv3x3s2_dgrad_kernel"):
        assert kernel in names, names


def test_adversarial_step_matches_the_reference_on_the_device():
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        rows, families, names = observed(lambda: C.check_step("cuda"))
    assert not [str(c.message) for c in caught if issubclass(c.category, RuntimeWarning)], [str(c.message) for c in caught]
    # enhanceNetSmall at 16 x 16 has two stride-2 layers.  Discriminator phase: 2 steps x 3 frames x 2 inputs (ground truth, prediction)
    # forward, and ONE deferred weight-gradient pass per layer and step over the six recorded pairs; the first layer of the network
    # needs no input gradient there.  Generator phase: 2 steps x 3 frames forward and data gradient, no weight gradient.
    assert names.count("conv3x3s2_fwd_kernel") == 2 * (2 * 3 * 2 + 2 * 3), names.count("conv3x3s2_fwd_kernel")
    assert names.count("conv3x3s2_wgrad_kernel") == 2 * 2, names.count("conv3x3s2_wgrad_kernel")
    assert names.count("conv3x3s2_dgrad_kernel") == 2 * (2 * 3 * 2 + 2 * 3), names.count("conv3x3s2_dgrad_kernel")
    assert families.get("exact", 0) > 0
