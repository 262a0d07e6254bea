"""CPU: the colour (shaded) networks of the reference through ``inference.LoadedModel`` -- RGB + mask (+ normal, depth) in, RGB out
(SuperresolutionNetwork/inference/loadedmodel.py:36-64,97-118) -- against frames produced by the reference's own modules
(tests/golden/make_colour_fixtures.py)."""
import numpy as np
import pytest
import torch

from colour_common import FRAMES, G, VARIANTS, colour_net, previous_of
from isosurfacesuperresolution_amd import models
from isosurfacesuperresolution_amd.inference import LoadedModel


@pytest.mark.parametrize("c,normal,depth", [(8, True, True), (7, True, False), (5, False, True), (4, False, False)])
def test_loaded_model_accepts_colour_networks(c, normal, depth):
    lm = LoadedModel.from_model(colour_net(c), "cpu")
    assert lm.unshaded is False and lm.input_channels == c + 48
    assert (lm.has_normal, lm.has_depth, lm.input_single_channels) == (normal, depth, 4)
    assert lm.initial_image_mode == "zero"                                   # loadedmodel.py:58-64
    assert LoadedModel.from_model(colour_net(c), "cpu", parameters={"initialImage": "input"}).initial_image_mode == "input"


def test_unshaded_networks_keep_their_defaults():
    from colour_common import OPT
    lm = LoadedModel.from_model(models.createNetwork('EnhanceNet', 4, 101, [0, 1, 2, 3, 4], 6, OPT), "cpu")
    assert lm.unshaded is True and lm.initial_image_mode == "input"


@pytest.mark.parametrize("c,mode", VARIANTS)
def test_inference_reproduces_the_reference_frame_by_frame(c, mode):
    """Teacher-forced: frame k runs from the fixture's clamped frame k - 1.  Tolerances: those tests/test_sr_golden_cpu.py applies to
    ``vt_warp_plain`` (2e-5: the explicit warp is a re-rounding of the reference's) and to the network output (1e-5)."""
    tag = "c%d_%s" % (c, mode)
    lm = LoadedModel.from_model(colour_net(c), "cpu", parameters={"initialImage": mode})
    seen = {}
    hook = lm.model.register_forward_pre_hook(lambda m, i: seen.__setitem__("x", i[0].detach().clone()))
    try:
        for k in range(FRAMES):
            low = torch.from_numpy(G["low"][k:k + 1])
            pred = lm.inference(low, previous_of(tag, k))
            assert pred.shape == (1, 3, 4 * low.shape[2], 4 * low.shape[3])
            np.testing.assert_allclose(seen["x"].numpy()[0], G[tag + "_input"][k], rtol=0, atol=2e-5)
            np.testing.assert_allclose(pred.numpy()[0], G[tag + "_prediction"][k], rtol=0, atol=1e-5)
    finally:
        hook.remove()


def test_the_package_fills_the_fixture_flows():
    from isosurfacesuperresolution_amd.inference.flowfill import fill_flow
    low = torch.from_numpy(G["low"])
    assert np.array_equal(fill_flow(low[:, 8:10], low[:, 3:4] != 0).numpy(), G["flow_filled"])


def test_unshaded_initial_image_has_no_three_channel_form():
    lm = LoadedModel.from_model(colour_net(8), "cpu", parameters={"initialImage": "unshaded"})
    with pytest.raises(ValueError):
        lm.inference(torch.from_numpy(G["low"][0:1]), None)


def test_pipeline_feeds_back_the_clamped_prediction():
    """``superresolve``: (mainVideo.py:416) the clamped prediction is what is displayed and what the next frame warps."""
    from isosurfacesuperresolution_amd.pipeline import SuperResolutionPipeline, fused_path_ok

    class NoRenderer:
        def send_command(self, *a):
            pass

    class NoShading:
        def get_fov(self):
            return 30.0
    lm = LoadedModel.from_model(colour_net(8), "cpu")
    assert fused_path_ok(lm)
    pipe = SuperResolutionPipeline(NoRenderer(), lm, NoShading(), (12, 8), device="cpu", fused=False, graph=True)
    assert pipe.colour and not pipe.graph and not pipe.fused
    for k in range(2):
        out = pipe.superresolve(torch.from_numpy(G["low"][k:k + 1]))
        assert out.shape == (1, 3, 32, 48) and out.min() >= 0 and out.max() <= 1 and pipe.previous is out
        np.testing.assert_allclose(out.numpy()[0], np.clip(G["c8_zero_prediction"][k], 0, 1), rtol=0, atol=1e-5 if k == 0 else 1e-4)


def test_strip_super_resolution_and_stats_refuse_colour_models():
    from isosurfacesuperresolution_amd import parallel_sr, stats
    lm = LoadedModel.from_model(colour_net(4), "cpu")
    with pytest.raises(NotImplementedError):
        parallel_sr.StripSuperResolution(lm, None)
    with pytest.raises(NotImplementedError):
        stats.load_models([{"name": "colour", "model": lm.model}], "cpu")
