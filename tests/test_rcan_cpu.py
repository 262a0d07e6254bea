"""CPU: the RCAN generator (``models.RCAN``, ``createNetwork('RCAN', ...)``) against frames produced by the reference's own module
(tests/golden/make_rcan_fixtures.py), its ``state_dict`` layout, the loading routes, and the new entry points of the kernel library."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rcan_common import CASES, G, PREMISE, SEQ, rcan_net, small_rcan
from isosurfacesuperresolution_amd import _native, models, ops
from isosurfacesuperresolution_amd.inference import LoadedModel


@pytest.fixture(scope="module")
def nets():
    return {case: rcan_net(case) for case in CASES}


@pytest.mark.parametrize("case", ["a", "b"])
def test_rcan_reproduces_the_reference(nets, case):
    """Every stored frame single-step from the stored network input through the CPU branch of the three new ops (their definition):
    prediction, unclamped output and the tensor after ``net.rir`` <= 1e-6; the frame-0 gates <= 1e-6."""
    net = nets[case]
    assert max(G[case + "_cpu32_vs_fp64_single_step"].max(), G[case + "_rir_cpu32_vs_fp64_single_step"].max()) <= PREMISE
    with torch.no_grad():
        for k in range(G[case + "_input"].shape[0]):
            x = torch.from_numpy(G[case + "_input"][k:k + 1])
            gates = []
            rir = net.forward_features(x, gates=gates)
            post = net.net['post']
            raw = ops.pixel_shuffle4_conv(rir, post.weight, post.bias)
            pred, residual = net(x)
            assert pred.shape == (1, 3, 32, 48) and rir.shape == (1, 64, 8, 12) and len(gates) == 200
            np.testing.assert_allclose(rir.numpy()[0], G[case + "_rir"][k], rtol=0, atol=1e-6)
            np.testing.assert_allclose(raw.numpy()[0], G[case + "_output"][k], rtol=0, atol=1e-6)
            np.testing.assert_allclose(pred.numpy()[0], G[case + "_prediction"][k], rtol=0, atol=1e-6)
            assert torch.equal(pred, torch.clamp(raw, 0, 1))
            assert torch.equal(residual, raw - F.interpolate(x[:, [0, 1, 2]], size=(32, 48), mode='bilinear'))
            if k == 0:
                np.testing.assert_allclose(torch.cat(gates).numpy(), G[case + "_gates_frame0"], rtol=0, atol=1e-6)


@pytest.mark.parametrize("case", ["a", "b"])
def test_state_dict_keys_and_shapes_are_the_reference_s(nets, case):
    net = nets[case]
    ours = ["%s:%s" % (k, ",".join(str(d) for d in t.shape)) for k, t in net.state_dict().items()]
    assert ours == list(G[case + "_keys"]) and len(ours) == 1626
    stored = {k for k in vars(net) if not k.startswith("_") and k != "training"}
    assert stored == {"upscale_factor", "upsample", "num_blocks_g", "num_blocks_b", "num_channels", "channel_downscaling",
                      "reduced_channels", "channel_mask"}
    assert (net.num_blocks_g, net.num_blocks_b, net.num_channels, net.channel_downscaling, net.reduced_channels) == (10, 20, 64, 16, 4)
    assert net.upsample == 'pixelShuffle' and net.upscale_factor == 4


def test_from_state_dict_round_trip():
    """Cin, Cout and the group and block counts come from the keys and shapes."""
    src = small_rcan(3, 2, cin=53)
    net = models.RCAN.from_state_dict(src.state_dict(), [0, 1, 2]).eval()
    assert (net.num_blocks_g, net.num_blocks_b) == (3, 2) and len(net.net['rir'].blocks) == 3 and len(net.net['rir'].blocks[0].blocks) == 2
    assert net.net['pre'].in_channels == 53 and net.net['post'].out_channels == 3
    assert list(net.state_dict()) == list(src.state_dict())
    x = torch.rand(1, 53, 5, 7, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(net(x), src(x)))
    with pytest.raises(ValueError):
        models.RCAN.from_state_dict({"preblock.0.weight": torch.zeros(64, 56, 3, 3)}, [0, 1, 2])


@pytest.mark.parametrize("cin,normal,depth", [(56, True, True), (55, True, False), (53, False, True), (52, False, False)])
def test_whole_object_checkpoint_of_this_package_loads_through_loaded_model(cin, normal, depth, tmp_path):
    """The block classes live at module level: a whole-object pickle of THIS package's RCAN does not go through ``getattr`` (the
    reference's nested classes do, and stay refused) and loads through the restricted unpickler; the model is classified as colour."""
    from isosurfacesuperresolution_amd.pipeline import fused_path_ok
    net = small_rcan(2, 2, cin=cin)
    path = str(tmp_path / "generator_RCAN.pth")
    torch.save({'model': net, 'parameters': {}}, path)
    lm = LoadedModel(path, "cpu", 4)
    assert isinstance(lm.model, models.RCAN) and lm.input_channels == cin and not lm.unshaded
    assert (lm.has_normal, lm.has_depth) == (normal, depth) and lm.initial_image_mode == "zero"
    assert fused_path_ok(lm)
    low = torch.from_numpy(SEQ["low"][0:1])
    with torch.no_grad():
        assert torch.equal(lm.inference(low, None), LoadedModel.from_model(net, "cpu").inference(low, None))


def test_five_mask_six_outputs_raises_not_implemented():
    """The reference's own forward cannot run the unshaded configuration (it subtracts five resized channels from six outputs)."""
    with pytest.raises(NotImplementedError, match="reference's own forward"):
        models.createNetwork('RCAN', 4, 101, [0, 1, 2, 3, 4], 6, None)
    with pytest.raises(NotImplementedError):
        models.createNetwork('SubpixelNet', 4, 56, [0, 1, 2], 3, None)
    assert isinstance(models.createNetwork('RCAN', 4, 56, [0, 1, 2], 3, None), models.RCAN)


def test_gathered_mask():
    """The second return value subtracts the input channels gathered by index (not sliced)."""
    net = small_rcan(1, 1, cin=8)
    net.channel_mask = [2, 0, 1]
    x = torch.rand(1, 8, 4, 6, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        pred, residual = net(x)
        post = net.net['post']
        raw = ops.pixel_shuffle4_conv(net.forward_features(x), post.weight, post.bias)
    assert torch.equal(residual, raw - F.interpolate(x[:, [2, 0, 1]], size=(16, 24), mode='bilinear'))
    assert not torch.equal(residual, raw - F.interpolate(x[:, [0, 1, 2]], size=(16, 24), mode='bilinear'))
    assert torch.equal(pred, raw.clamp(0, 1))


def test_op_definitions_on_the_cpu():
    """The CPU branch of each op is its definition in plain torch."""
    g = torch.Generator().manual_seed(3)
    x, t = torch.randn(2, 64, 5, 7, generator=g), torch.randn(2, 64, 5, 7, generator=g)
    wd, bd, wu, bu = torch.randn(4, 64, generator=g), torch.randn(4, generator=g), torch.randn(64, 4, generator=g), torch.randn(64, generator=g)
    z = ops.channel_pool(t)
    assert torch.equal(z, t.view(2, 64, 35).mean(dim=2))
    s = torch.sigmoid(F.linear(F.leaky_relu(F.linear(z, wd, bd), 0.2), wu, bu))
    y, gate = ops.channel_attention_residual(x, t, wd, bd, wu, bu, slope=0.2, return_gate=True)
    assert torch.equal(gate, s) and torch.equal(y, x + t * s[:, :, None, None])
    assert torch.equal(ops.channel_attention_residual(x, t, wd, bd, wu, bu, slope=0.2), y)
    w, b = torch.randn(3, 4, 3, 3, generator=g), torch.randn(3, generator=g)
    want = F.conv2d(F.pixel_shuffle(x, 4), w, b, padding=1)
    assert torch.equal(ops.pixel_shuffle4_conv(x, w, b), want)
    assert torch.equal(ops.pixel_shuffle4_conv(x, w, b, clamp=True), want.clamp(0, 1))
    assert not ops.channel_pool_supported(t) and not ops.pixel_shuffle4_conv_supported(x, w)          # CPU tensors: not the kernels' business


def test_new_symbols_are_exported_with_their_ctypes_signatures():
    _native.build()
    vp, ci, cf, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
    want = {"isrChannelPoolSlabs": [ci, ci, ci],
            "isrChannelPoolSupported": [ci, ci, ci, ci, ll, ll],
            "isrChannelGateScaleAddSupported": [ci, ci, ci, ci, ci, ll, ll],
            "isrChannelPool": [vp, ll, ll, ci, ci, ci, ci, ci, vp, vp],
            "isrChannelPoolMean": [vp, ci, ci, ci, ci, ci, vp, vp],
            "isrChannelGateScaleAdd": [vp, vp, vp, ll, ll, ll, ll, ll, ll, vp, ci, vp, vp, vp, vp, cf, vp, ci, ci, ci, ci, ci, vp],
            "isrShuffleTailColourSupported": [ci, ci, ci, ci, ci, ll, ll, ll, ll],
            "isrShuffleTailColour": [vp, ll, ll, vp, vp, vp, ll, ll, ci, ci, ci, ci, ci, ci, vp]}
    header = open(_native.CSRC + "/../../include/isr_sr_kernels.h").read()
    for path in (_native.LIBDIR + "/libisr_sr.so", _native.SR_DIAG_LIB):
        lib = ops._bind(_native.load(path))
        for name, argtypes in want.items():
            fn = getattr(lib, name)
            assert list(fn.argtypes) == argtypes and fn.restype is ci, name
            assert name + "(" in header, name
    lib = ops._bind(_native.load(_native.LIBDIR + "/libisr_sr.so"))
    # the predicates and the slab rule are host code: C = 64 with 4 reduced channels, one image below 2 GiB; S = 1 at tiny sizes, > 1 at 67 x 129
    assert lib.isrChannelGateScaleAddSupported(1, 64, 4, 270, 480, 270 * 480, 64 * 270 * 480) == 1
    assert lib.isrChannelPoolSupported(1, 64, 270, 480, 270 * 480, 64 * 270 * 480) == 1
    assert lib.isrChannelPoolSupported(1, 32, 8, 8, 64, 32 * 64) == 0 and lib.isrChannelGateScaleAddSupported(1, 64, 8, 8, 8, 64, 64 * 64) == 0
    assert lib.isrChannelPoolSupported(1, 64, 4096, 4096, 4096 * 4096, 64 * 4096 * 4096) == 0          # an image of 4 GiB
    assert lib.isrChannelGateScaleAddSupported(1, 64, 4, 4096, 4096, 4096 * 4096, 64 * 4096 * 4096) == 0
    assert lib.isrChannelPoolSupported(1, 64, 8, 8, 63, 64 * 63) == 0                                   # planes that overlap
    assert lib.isrChannelPoolSlabs(2, 8, 12) == 1 and lib.isrChannelPoolSlabs(1, 1, 1) == 1 and lib.isrChannelPoolSlabs(2, 67, 129) > 1
    assert 1024 <= 64 * lib.isrChannelPoolSlabs(1, 270, 480) <= 4096
    assert lib.isrShuffleTailColourSupported(1, 64, 3, 270, 480, 270 * 480, 64 * 270 * 480, 1080 * 1920, 3 * 1080 * 1920) == 1
    assert lib.isrShuffleTailColourSupported(1, 64, 9, 8, 8, 64, 64 * 64, 1024, 9 * 1024) == 0
    assert lib.isrShuffleTailColourSupported(1, 48, 3, 8, 8, 64, 48 * 64, 1024, 3 * 1024) == 0
    assert {39: "channel_pool_kernel", 40: "gate_scale_add_kernel", 41: "shuffle_tail_kernel"}.items() <= ops.VARIANT_NAMES.items()
