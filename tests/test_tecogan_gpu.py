"""GPU: the TecoGAN generator on the HIP kernels -- the module on the device, the fused colour frame
(``ops.assemble_input_colour`` -> ``pipeline.run_network_colour``) and ``SuperResolutionPipeline`` -- against frames of the reference
itself (tests/golden/make_tecogan_fixtures.py) and against the module route on the same device."""
import numpy as np
import pytest
import torch

from tecogan_common import BOUND, CASES, G, PREMISE, SEQ, tecogan_net

pytestmark = pytest.mark.gpu

CONVT = "convt3x3s2_split_kernel"


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_module_on_the_device_matches_the_reference(case):
    """Every stored frame single-step from the stored network input: <= 1e-4, on the premise -- recorded in the fixture -- that the
    reference's fp32 is within 4e-5 of fp64.  Both transposed convolutions run on the new kernel."""
    from isosurfacesuperresolution_amd import ops
    assert G[case + "_cpu32_vs_fp64_single_step"].max() <= PREMISE
    ops.range_reset()
    net = tecogan_net(case).cuda()
    with torch.no_grad():
        for k in range(G[case + "_input"].shape[0]):
            ops.profile_enable(True)
            try:
                recon, outputs = net(torch.from_numpy(G[case + "_input"][k:k + 1]).cuda())
                torch.cuda.synchronize()
                names = [n for n, _, _ in ops.profile_records()]
            finally:
                ops.profile_enable(False)
            assert names.count(CONVT) == 2, names
            err = np.abs(recon.cpu().numpy()[0] - G[case + "_prediction"][k]).max()
            print("tecogan %s frame %d: %.3g" % (case, k, err))
            assert err <= BOUND, (case, k, err)
    assert not ops.refresh_range_flags("cuda") and not ops.any_hot("cuda")


def test_fused_colour_frames():
    """Case (a) through the kernels ``SuperResolutionPipeline(fused=True)`` launches, the recurrence fed by the fused route's own
    output: the first frame against the fixture (<= 1e-4; later frames are not single-step), every frame against the module route on
    the same device -- ``LoadedModel.inference`` + clamp from the same previous frame.  The two routes run the same layer kernels on
    bit-identical inputs (tests/test_colour_gpu.py: the assembly, and the finishing = ``ops.recon_residual`` + clamp): ``torch.equal``."""
    from isosurfacesuperresolution_amd import ops
    from isosurfacesuperresolution_amd.inference import LoadedModel
    from isosurfacesuperresolution_amd.pipeline import fused_path_ok, run_network_colour
    lm = LoadedModel.from_model(tecogan_net("a"), "cuda")
    assert fused_path_ok(lm) and not lm.unshaded and lm.input_channels == 56
    prev = None
    with torch.no_grad():
        for k in range(SEQ["low"].shape[0]):
            low = torch.from_numpy(SEQ["low"][k:k + 1]).cuda()
            gb = low[0].permute(1, 2, 0).contiguous()
            flow = ops.fill_flow_gbuffer(gb) if prev is not None else None
            x = ops.assemble_input_colour(gb, flow, prev, 8, lm.initial_image_mode)
            frame = run_network_colour(lm, x)
            module = lm.inference(low, prev).clamp(0, 1)
            torch.cuda.synchronize()
            assert frame.shape == (1, 3, 32, 48)
            diff = (frame - module).abs().max().item()
            print("fused tecogan frame %d: against the module route %.3g" % (k, diff))
            assert diff <= 1e-6
            assert torch.equal(frame, module)
            if k == 0:
                err = np.abs(frame.cpu().numpy()[0] - np.clip(G["a_prediction"][0], 0, 1)).max()
                print("fused tecogan frame 0: against the fixture %.3g" % err)
                assert err <= BOUND
            prev = frame
    ops.guards_flush("cuda")


def _pipeline(lm, fused=True):
    import render_scenes
    from isosurfacesuperresolution_amd.inference import DirectRenderer
    from isosurfacesuperresolution_amd.pipeline import SuperResolutionPipeline, default_shading
    renderer = DirectRenderer()
    renderer.load_dense(render_scenes.scene_a()[0])
    pipe = SuperResolutionPipeline(renderer, lm, default_shading("cuda", 45.0), (48, 32), fused=fused)
    pipe.set_static(fov=45.0, isovalue=0.5)
    return pipe


def test_pipeline_with_a_colour_tecogan_is_fused():
    from isosurfacesuperresolution_amd import ops, volumes as V
    from isosurfacesuperresolution_amd.inference import LoadedModel
    pipe = _pipeline(LoadedModel.from_model(tecogan_net("a"), "cuda"))
    assert pipe.fused and pipe.colour and not pipe.graph
    for k in range(2):
        ops.profile_enable(True)
        try:
            rgb, raw = pipe.frame(V.orbit_camera(k))
            torch.cuda.synchronize()
            names = [n for n, _, _ in ops.profile_records()]
        finally:
            ops.profile_enable(False)
        assert names.count(CONVT) == 2, names
        assert rgb.shape == (1, 3, 128, 192) and torch.equal(rgb, raw)
        assert rgb.min().item() >= 0 and rgb.max().item() <= 1 and torch.isfinite(rgb).all()
    assert (pipe.gbuffer[..., 3] != 0).any()                       # the scene is in view: the frame is not a frame of background
    pipe.close()


def test_pipeline_with_an_unshaded_direct_tecogan_takes_the_module_route():
    from isosurfacesuperresolution_amd import ops, volumes as V
    from isosurfacesuperresolution_amd.inference import LoadedModel
    pipe = _pipeline(LoadedModel.from_model(tecogan_net("c"), "cuda"))
    assert not pipe.fused and not pipe.colour
    ops.profile_enable(True)
    try:
        rgb, raw = pipe.frame(V.orbit_camera(0))
        torch.cuda.synchronize()
        names = [n for n, _, _ in ops.profile_records()]
    finally:
        ops.profile_enable(False)
    assert names.count(CONVT) == 2, names
    assert rgb.shape == (1, 3, 128, 192) and raw.shape == (1, 6, 128, 192) and torch.isfinite(rgb).all() and torch.isfinite(raw).all()
    pipe.close()


@pytest.mark.parametrize("upsample,recon", [("nearest", "residual"), ("bilinear", "direct")])
def test_other_colour_tecogans_take_the_module_route(upsample, recon):
    """A colour TecoGAN with another resize mode, or direct reconstruction: not the fused frame path; ``LoadedModel.inference`` with
    the layers on the HIP kernels, against the same network on the CPU."""
    import argparse
    from isosurfacesuperresolution_amd import models
    from isosurfacesuperresolution_amd.inference import LoadedModel
    from isosurfacesuperresolution_amd.pipeline import fused_path_ok
    from tecogan_common import fill_state_dict
    opt = argparse.Namespace(upsample=upsample, reconType=recon, useBN=False, numResidualLayers=2)
    nets = [fill_state_dict(models.createNetwork('TecoGAN', 4, 56, [0, 1, 2], 3, opt).eval(), 5) for _ in range(2)]
    lm, ref = LoadedModel.from_model(nets[0], "cuda"), LoadedModel.from_model(nets[1], "cpu")
    assert not fused_path_ok(lm)
    low = torch.from_numpy(SEQ["low"][0:1])
    with torch.no_grad():
        out = lm.inference(low.cuda(), None)
        want = ref.inference(low, None)
    assert (out.cpu() - want).abs().max().item() <= BOUND
