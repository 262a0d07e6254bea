"""CPU: the TecoGAN generator (``models.TecoGAN``, ``createNetwork('TecoGAN', ...)``) against frames produced by the reference's own
module (tests/golden/make_tecogan_fixtures.py), its ``state_dict`` layout, the pickled-whole-object checkpoint route through
``inference.LoadedModel``, and what stays as it was."""
import argparse

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tecogan_common import CASES, G, SEQ, options, tecogan_net
from isosurfacesuperresolution_amd import models, ops
from isosurfacesuperresolution_amd.inference import LoadedModel


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_tecogan_reproduces_the_reference(case):
    """Every stored frame single-step from the stored network input: 1e-5 (the tolerance tests/test_sr_golden_cpu.py applies to a
    network output on the CPU)."""
    net = tecogan_net(case)
    with torch.no_grad():
        for k in range(G[case + "_input"].shape[0]):
            recon, outputs = net(torch.from_numpy(G[case + "_input"][k:k + 1]))
            assert recon.shape == (1, CASES[case]["cout"], 32, 48)
            np.testing.assert_allclose(recon.numpy()[0], G[case + "_prediction"][k], rtol=0, atol=1e-5)
            if CASES[case]["recon"] == "direct":
                assert recon is outputs


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_state_dict_keys_and_shapes_are_the_reference_s(case):
    net = tecogan_net(case)
    ours = ["%s:%s" % (k, ",".join(str(d) for d in t.shape)) for k, t in net.state_dict().items()]
    assert ours == list(G[case + "_keys"])
    assert len(net.blocks) == CASES[case]["blocks"]


def test_conv_transpose_op_on_the_cpu_and_its_phase_form():
    """``ops.conv_transpose3x3_s2`` on CPU tensors is PyTorch's operator + the activation; the zero-embedded phase weight of the exact
    device route (3x3 convolution to 4 Cout channels + pixel shuffle) is the same function (fp64: rounding-level agreement)."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 5, 3, 7, generator=g, dtype=torch.float64)
    w = torch.randn(5, 6, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(6, generator=g, dtype=torch.float64)
    ref = F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1)
    assert torch.equal(ops.conv_transpose3x3_s2(x, w, b), ref)
    assert torch.equal(ops.conv_transpose3x3_s2(x, w, b, act='leaky', slope=0.5), F.leaky_relu(ref, 0.5))
    we = ops.conv_transpose_phase_weight(w)
    assert we.shape == (24, 5, 3, 3) and int((we != 0).sum()) == 9 * 5 * 6
    y = F.pixel_shuffle(F.conv2d(x, we, b.repeat_interleave(4), padding=1), 2)
    assert (y - ref).abs().max().item() <= 1e-13
    with pytest.raises(ValueError):
        ops.conv_transpose3x3_s2(x, w.permute(1, 0, 2, 3).contiguous(), b)


def _reference_like_object(case):
    """A TecoGAN as unpickling a REFERENCE checkpoint leaves it: ``__init__`` bypassed, only the reference's five attributes (and the
    sub-modules) present."""
    src = tecogan_net(case)
    net = models.TecoGAN.__new__(models.TecoGAN)
    torch.nn.Module.__init__(net)
    net.upscale_factor, net.upsample, net.recon_type = 4, src.upsample, src.recon_type
    net.num_residual_layers, net.channel_mask = src.num_residual_layers, src.channel_mask
    net.preblock, net.blocks, net.postblock = src.preblock, src.blocks, src.postblock
    own = {k for k in vars(net) if not k.startswith("_") and k != "training"}
    assert own == {"upscale_factor", "upsample", "recon_type", "num_residual_layers", "channel_mask"}
    return net.eval()


@pytest.mark.parametrize("case", ["a", "c"])
def test_pickled_whole_object_loads_through_loaded_model(case, tmp_path):
    """The reference saves ``{'model': net, 'parameters': ...}`` with the whole module pickled (as ``models.tecogan.TecoGAN``; here the
    package's own module path, which the restricted unpickler resolves the same way): it loads, is classified by its first
    convolution, and ``inference`` gives the frame the in-memory object gives."""
    from isosurfacesuperresolution_amd.pipeline import fused_path_ok
    path = str(tmp_path / ("generator_TecoGAN_%s.pth" % case))
    torch.save({'model': _reference_like_object(case), 'parameters': {}}, path)
    lm = LoadedModel(path, "cpu", 4)
    assert isinstance(lm.model, models.TecoGAN) and lm.input_channels == CASES[case]["cin"]
    assert lm.unshaded is (case == "c")
    assert fused_path_ok(lm) is (case == "a")
    low = torch.from_numpy(SEQ["low"][0:1])
    direct = LoadedModel.from_model(tecogan_net(case), "cpu").inference(low, None)
    assert torch.equal(lm.inference(low, None), direct)
    assert direct.shape == (1, CASES[case]["cout"], 32, 48)
    if case == "a":          # the colour family: the first frame starts from zeros -- the stored input, the stored prediction
        np.testing.assert_allclose(direct.numpy()[0], G["a_prediction"][0], rtol=0, atol=1e-5)


def test_reference_module_path_in_a_pickle_resolves_to_this_package(tmp_path):
    """A checkpoint written by the reference names ``models.tecogan.TecoGAN``: the restricted unpickler maps ``models.*`` to this package."""
    from isosurfacesuperresolution_amd.inference.loadedmodel import _CheckpointPickle
    import io
    import pickle
    cls = _CheckpointPickle.Unpickler(io.BytesIO(pickle.dumps(0))).find_class("models.tecogan", "TecoGAN")
    assert cls is models.TecoGAN


def test_residual_tecogan_needs_as_many_outputs_as_masked_inputs():
    """tecogan.py:30-35 adds the resized masked input to the whole output: mask [0..4] with 6 outputs raises in the reference (a size
    mismatch) and here."""
    opt = argparse.Namespace(upsample='bilinear', reconType='residual', useBN=False, numResidualLayers=1)
    net = models.createNetwork('TecoGAN', 4, 101, [0, 1, 2, 3, 4], 6, opt).eval()
    with torch.no_grad(), pytest.raises(RuntimeError):
        net(torch.zeros(1, 101, 4, 4))


def test_gathered_mask_and_other_modes_take_the_plain_route():
    """The input channels are gathered by index (not sliced): a permuted mask, and a mode other than bilinear."""
    opt = argparse.Namespace(upsample='nearest', reconType='residual', useBN=False, numResidualLayers=1)
    torch.manual_seed(0)
    net = models.createNetwork('TecoGAN', 4, 8, [2, 0, 5], 3, opt).eval()
    x = torch.rand(1, 8, 4, 6)
    with torch.no_grad():
        recon, outputs = net(x)
    assert torch.equal(recon, F.interpolate(x[:, [2, 0, 5]], scale_factor=4, mode='nearest') + outputs)


def test_other_generators_still_raise():
    for name in ('RCAN', 'SubpixelNet'):
        with pytest.raises(NotImplementedError):
            models.createNetwork(name, 4, 101, [0, 1, 2, 3, 4], 6, options("c"))
    with pytest.raises(ValueError):
        models.createNetwork('nonesuch', 4, 101, [0, 1, 2, 3, 4], 6, options("c"))
