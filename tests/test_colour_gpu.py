"""GPU: the colour (shaded) networks on the HIP frame path -- input assembly (isrAssembleInputColour), the colour finishing standalone,
behind the small-Cout last layer and behind the three-channel fused tail (isrConvTailFinishFrame3), the routing of
``pipeline.run_network_colour`` -- against the module path, an fp64 evaluation and frames of the reference itself
(tests/golden/make_colour_fixtures.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from colour_common import BOUND, FRAMES, G, OPT, PREMISE, VARIANTS, colour_net, previous_of

pytestmark = pytest.mark.gpu

UPS_KERNELS = {"conv3x3_split_ups3_kernel", "conv3x3_split_ups4_kernel", "conv3x3_split_kernel<true>"}
TRUNK_KERNELS = {"trunk_dataflow_kernel", "trunk_mt_kernel"}
UNSHADED_FRAME_KERNELS = {"conv3x3_split_tail_kernel", "tail_finish_kernel", "finish_frame_kernel", "assemble_input_kernel"}


def _gbuffer(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    gb = torch.rand((h, w, 12), generator=g) * 1.3 - 0.15                 # colours / normals outside [0, 1]: the c = 8 clamp acts
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    gb[..., 3] = (((yy - 0.45 * h) ** 2 + (xx - 0.55 * w) ** 2) < (0.3 * min(h, w)) ** 2).float()
    gb[..., 8:10] = (torch.rand((h, w, 2), generator=g) - 0.5) * 0.04
    return gb


def _loaded(c, mode="zero", device="cuda", seed=None):
    from isosurfacesuperresolution_amd.inference import LoadedModel
    return LoadedModel.from_model(colour_net(c, seed), device, parameters={"initialImage": mode})


@pytest.mark.parametrize("h,w", [(24, 40), (23, 37)])
@pytest.mark.parametrize("c", [8, 7, 5, 4])
def test_colour_assembly_is_bit_identical_to_the_module_path(c, h, w):
    """Channel selection (with the clamp for c = 8 only), warp of the previous RGB frame (zero padding, no mask remap), space-to-depth:
    ``ops.assemble_input_colour`` against ``LoadedModel.colour_network_input`` on the device AND on the CPU, with a previous frame that
    has hard edges, without one for both initial modes (the reference warps the initial image too), at an aligned and a ragged size."""
    from isosurfacesuperresolution_amd import ops
    gb = _gbuffer(h, w, seed=c * 1000 + h * 7 + w)
    H, W = 4 * h, 4 * w
    YY, XX = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    inside = (((YY - 0.5 * H) ** 2 + (XX - 0.5 * W) ** 2) < (0.33 * min(H, W)) ** 2).float()
    prev = torch.rand((1, 3, H, W), generator=torch.Generator().manual_seed(c)) * inside
    gb_d = gb.cuda()
    flow_d = ops.fill_flow_gbuffer(gb_d)
    for mode, p in (("zero", prev), ("zero", None), ("input", None), ("input", prev)):
        x = ops.assemble_input_colour(gb_d, flow_d if (p is not None or mode == "input") else None, None if p is None else p.cuda(), c, mode)
        torch.cuda.synchronize()
        assert x.shape == (1, c + 48, h, w)
        for dev in ("cuda", "cpu"):
            lm = _loaded(c, mode, dev)
            low = gb.permute(2, 0, 1).unsqueeze(0).to(dev)
            with torch.no_grad():
                ref = lm.colour_network_input(low, None if p is None else p.to(dev))
            assert torch.equal(x.cpu(), ref.cpu()), (mode, p is not None, dev, (x.cpu() - ref.cpu()).abs().max().item())
    with pytest.raises(ValueError):
        ops.assemble_input_colour(gb_d, flow_d, None, c, "unshaded")


@pytest.mark.parametrize("h,w", [(6, 8), (23, 37), (67, 120)])
def test_colour_finish_standalone_and_fused_equal_the_module_path(h, w):
    """clamp(recon_residual(conv output, input, 3), 0, 1): the standalone finishing kernel, the finishing in the small-Cout last
    layer's epilogue and the module path's ``ops.recon_residual`` + clamp, bit for bit."""
    from isosurfacesuperresolution_amd import ops
    g = torch.Generator().manual_seed(h * 11 + w)
    f6 = torch.rand(1, 64, 4 * h, 4 * w, generator=g).cuda()
    w8 = ((torch.rand(3, 64, 3, 3, generator=g) - 0.5) * 0.08).cuda()
    b8 = ((torch.rand(3, generator=g) - 0.5) * 0.1).cuda()
    x = (torch.rand(1, 56, h, w, generator=g) * 1.2 - 0.1).cuda()
    with torch.no_grad():
        raw = ops.conv3x3(f6, w8, b8)                                  # the small-Cout kernel
        module = torch.clamp(ops.recon_residual(raw, x, 3), 0, 1)
        alone = ops.finish_frame_colour(raw, x)
        fused = ops.final_conv_finish_colour(f6, w8, b8, x)
    torch.cuda.synchronize()
    assert ops.recon_residual_supported(raw, x, 3)
    assert 0.05 < ((module > 0) & (module < 1)).float().mean().item()          # (the clamp does not hide everything)
    assert torch.equal(alone, module), (alone - module).abs().max().item()
    assert torch.equal(fused, alone), (fused - alone).abs().max().item()
    ref = torch.clamp(raw.double().cpu() + F.interpolate(x.double().cpu()[:, :3], scale_factor=4, mode='bilinear', align_corners=False), 0, 1)
    assert (alone.double().cpu() - ref).abs().max().item() <= 1e-6


def _tail_setup(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    f4 = torch.rand(1, 64, 4 * h, 4 * w, generator=g).cuda()                    # post-ReLU features: non-negative
    w6 = ((torch.rand(64, 64, 3, 3, generator=g) - 0.5) * 0.08).cuda()
    b6 = ((torch.rand(64, generator=g) - 0.5) * 0.1).cuda()
    w8 = ((torch.rand(3, 64, 3, 3, generator=g) - 0.5) * 0.08).cuda()
    b8 = ((torch.rand(3, generator=g) - 0.5) * 0.1).cuda()
    x = torch.rand(1, 56, h, w, generator=g).cuda()
    return f4, w6, b6, w8, b8, x


def _tail_reference64(f4, w6, b6, w8, b8, x):
    d = lambda t: t.double().cpu()
    y6 = F.relu(F.conv2d(d(f4), d(w6), d(b6), padding=1))
    out = F.conv2d(y6, d(w8), d(b8), padding=1)
    out += F.interpolate(d(x)[:, :3], size=out.shape[2:], mode='bilinear', align_corners=False)
    return out.clamp(0, 1), out


@pytest.mark.parametrize("h,w", [(2, 8), (6, 8), (23, 37), (30, 52), (67, 120)])
def test_colour_tail_matches_the_three_kernel_path_and_fp64(h, w):
    """The criterion of test_tail_gpu.py::test_tail_matches_the_three_kernel_path_and_fp64, for three output channels."""
    from isosurfacesuperresolution_amd import ops
    f4, w6, b6, w8, b8, x = _tail_setup(h, w, seed=h * 100 + w)
    assert ops.tail_supported(f4, w6, w8)
    with torch.no_grad():
        out_t = ops.tail_conv_finish_colour(f4, w6, b6, w8, b8, x)
        f6 = ops.conv3x3(f4, w6, b6, act='relu')
        out_s = ops.final_conv_finish_colour(f6, w8, b8, x)
    torch.cuda.synchronize()
    ref, pre = _tail_reference64(f4, w6, b6, w8, b8, x)
    assert 0.05 < ((ref > 0) & (ref < 1)).float().mean().item()
    scale = max(1.0, pre.abs().max().item())
    err_t = (out_t.double().cpu() - ref).abs().max().item()
    err_s = (out_s.double().cpu() - ref).abs().max().item()
    print("colour tail %dx%d: err_t %.3g err_s %.3g scale %.3g" % (h, w, err_t, err_s, scale))
    assert err_s <= 2e-5 * scale, err_s
    assert err_t <= 2e-5 * scale and err_t <= 4 * err_s + 2e-6, (err_t, err_s)
    assert (out_t - out_s).abs().max().item() <= 2e-5 * scale
    assert torch.isfinite(out_t).all()


@pytest.mark.parametrize("h,w", [(4, 8), (11, 20), (30, 52), (135, 240)])
def test_colour_tail_packed_split_input_is_bit_identical(h, w):
    from isosurfacesuperresolution_amd import ops
    f4, w6, b6, w8, b8, x = _tail_setup(h, w, seed=h * 13 + w)
    assert ops.packed_supported(f4, w6, False)
    with torch.no_grad():
        a = ops.tail_conv_finish_colour(f4, w6, b6, w8, b8, x)
        b = ops.tail_conv_finish_colour(ops.pack_split(f4), w6, b6, w8, b8, x)
        a2 = ops.tail_conv_finish_colour(f4, w6, b6, w8, b8, x)
        none = ops.tail_conv_finish_colour(f4, w6, None, w8, None, x)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, a2)
    ref, _ = _tail_reference64(f4, w6, torch.zeros_like(b6), w8, torch.zeros_like(b8), x)
    assert (none.double().cpu() - ref).abs().max().item() <= 2e-5


def test_colour_tail_does_not_depend_on_where_tile_borders_fall():
    """In the style of test_tail_gpu.py::test_s_form_does_not_depend_on_where_tile_borders_fall: crops at horizontal offsets 0 .. 32
    and two vertical ones, all three channels (the low-resolution input is cropped with the features, so the reconstruction's taps
    agree two pixels inside)."""
    from isosurfacesuperresolution_amd import ops
    h, w = 24, 40
    f4, w6, b6, w8, b8, x = _tail_setup(h, w, seed=21)
    with torch.no_grad():
        full = ops.tail_conv_finish_colour(f4, w6, b6, w8, b8, x)
        for oy in (0, 4):
            for ox in range(0, 36, 4):
                part = ops.tail_conv_finish_colour(f4[:, :, oy:, ox:].contiguous(), w6, b6, w8, b8, x[:, :, oy // 4:, ox // 4:].contiguous())
                assert torch.equal(full[:, :, oy + 2:-2, ox + 2:-2], part[:, :, 2:-2, 2:-2]), (oy, ox)
    assert 0.05 < ((full > 0) & (full < 1)).float().mean().item()


def _fused_frame(lm, low, prev, c, mode):
    """One fixture frame through the kernels ``SuperResolutionPipeline(fused=True)`` launches: assemble -> run_network."""
    from isosurfacesuperresolution_amd import ops
    from isosurfacesuperresolution_amd.pipeline import run_network_colour
    gb = low[0].permute(1, 2, 0).contiguous().cuda()
    need_flow = prev is not None or mode == "input"
    flow = ops.fill_flow_gbuffer(gb) if need_flow else None
    x = ops.assemble_input_colour(gb, flow, None if prev is None else prev.cuda(), c, mode)
    return x, run_network_colour(lm, x)


@pytest.mark.parametrize("c,mode", VARIANTS)
def test_fused_colour_frames_match_the_reference(c, mode):
    """Single-step against the reference's own prediction (after the clamp), every frame, every pixel: <= 1e-4, on the premise --
    recorded in the fixture -- that the reference's fp32 is within 4e-5 of fp64."""
    from isosurfacesuperresolution_amd import ops
    tag = "c%d_%s" % (c, mode)
    assert G[tag + "_cpu32_vs_fp64_single_step"].max() <= PREMISE
    lm = _loaded(c, mode)
    with torch.no_grad():
        for k in range(FRAMES):
            low = torch.from_numpy(G["low"][k:k + 1])
            ops.profile_enable(True)
            x, frame = _fused_frame(lm, low, previous_of(tag, k), c, mode)
            torch.cuda.synchronize()
            names = {n for n, _, _ in ops.profile_records()}
            ops.profile_enable(False)
            assert "conv3x3_split_tail_colour_kernel" in names and names & TRUNK_KERNELS, names      # not through a fallback
            ref = np.clip(G[tag + "_prediction"][k], 0, 1)
            err_in = np.abs(x.cpu().numpy()[0] - G[tag + "_input"][k]).max()
            err = np.abs(frame.cpu().numpy()[0] - ref).max()
            print("%s frame %d: input %.3g output %.3g" % (tag, k, err_in, err))
            assert err_in <= 2e-5
            assert err <= BOUND, (tag, k, err)
    assert not ops.any_hot(frame.device)


def test_colour_frame_routing():
    """The frame runs the dataflow trunk, the split upsampling kernels (packed-split hand-over) and the COLOUR tail; no kernel of the
    unshaded frame and no small-Cout fallback."""
    from isosurfacesuperresolution_amd import ops
    from isosurfacesuperresolution_amd.pipeline import run_network_colour
    lm = _loaded(8)
    gb = _gbuffer(64, 96, seed=5).cuda()
    prev = torch.rand(1, 3, 256, 384, generator=torch.Generator().manual_seed(1)).cuda()
    with torch.no_grad():
        flow = ops.fill_flow_gbuffer(gb)
        x = ops.assemble_input_colour(gb, flow, prev, 8)
        assert ops.trunk_supported(x, lm.model.trunk_convs())
        run_network_colour(lm, x)                                    # (weight images prepared)
        ops.profile_enable(True, small_kernels=True)
        x = ops.assemble_input_colour(gb, flow, prev, 8)
        frame = run_network_colour(lm, x)
        torch.cuda.synchronize()
        records = ops.profile_records()
        ops.profile_enable(False)
    names = [n for n, _, _ in records]
    assert names.count("assemble_input_colour_kernel") == 1 and len([n for n in names if n in TRUNK_KERNELS]) == 1
    assert len([n for n in names if n in UPS_KERNELS]) == 2, names
    assert names.count("conv3x3_split_tail_colour_kernel") == 1 and names.count("tail_finish_colour_kernel") == 1
    assert not (set(names) & UNSHADED_FRAME_KERNELS) and "conv3x3_small_cout_kernel" not in names and "finish_frame_colour_kernel" not in names
    assert frame.shape == (1, 3, 256, 384) and frame.min() >= 0 and frame.max() <= 1
    # and it is the module path's frame
    with torch.no_grad():
        ref = lm.model.double().cpu()(x.double().cpu())[0].clamp(0, 1)
    lm.model.float().cuda()
    assert (frame.double().cpu() - ref).abs().max().item() <= BOUND


def test_colour_checkpoint_with_a_badly_scaled_layer_takes_the_exact_route():
    """The range guard applies to the colour tail as to the unshaded one: a block-3 convolution scaled by 1e5 trips it on the first
    frame, the frame is computed again per layer on the exact kernels (small-Cout last layer with the colour finishing) and matches
    the fp64 CPU network; through ``LoadedModel.inference`` and through the frame pipeline."""
    from isosurfacesuperresolution_amd import ops, volumes as V
    from isosurfacesuperresolution_amd.inference import DirectRenderer, LoadedModel
    from isosurfacesuperresolution_amd.pipeline import SuperResolutionPipeline, default_shading
    net = colour_net(8, seed=31)
    with torch.no_grad():
        net.blocks[3][0].weight.mul_(1.0e5)
    ref_net = colour_net(8, seed=31).double()
    ref_net.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
    ref_lm = LoadedModel.from_model(ref_net, "cpu")
    lm = LoadedModel.from_model(net, "cuda")
    low = _gbuffer(24, 40, seed=6).permute(2, 0, 1).unsqueeze(0)
    with torch.no_grad():
        out = lm.inference(low.cuda(), None)
        ref = ref_lm.inference(low.double(), None)
    assert ops.any_hot(out.device)
    scale = ref.abs().max().item()
    assert scale > 1e4 and torch.isfinite(out).all()
    assert (out.double().cpu() - ref).abs().max().item() <= 1e-4 * scale
    renderer = DirectRenderer()
    renderer.load_dense(V.ejecta(64))
    lm2 = LoadedModel.from_model(net, "cuda")                          # resets the guard
    assert not ops.any_hot(out.device)
    pipe = SuperResolutionPipeline(renderer, lm2, default_shading("cuda", 30.0), (96, 56))
    pipe.set_static(fov=30.0, isovalue=0.34)
    rgb, raw = pipe.frame(V.orbit_camera(0))
    assert ops.any_hot(raw.device) and torch.isfinite(raw).all() and raw.shape[1] == 3
    # (the clamped frame of a network whose outputs are 1e4 .. 1e7 cannot be held to an absolute bound against fp64: a relative 1e-4
    # before the clamp is anything inside [0, 1] after it.)  What can be said exactly: with the layer marked hot the pipeline's frame
    # -- HIP assembly, per-layer exact route, the finishing in the last layer's epilogue -- is the module path's frame on the same
    # G-buffer (torch assembly, the same layers, ops.recon_residual, clamp), bit for bit.
    with torch.no_grad():
        module = lm2.inference(pipe.gbuffer.permute(2, 0, 1).unsqueeze(0), None).clamp(0, 1)
    assert torch.equal(raw, module), (raw - module).abs().max().item()
    ops.profile_enable(True)
    rgb2, raw2 = pipe.frame(V.orbit_camera(1))
    torch.cuda.synchronize()
    names = {n for n, _, _ in ops.profile_records()}
    ops.profile_enable(False)
    assert "conv3x3_small_cout_kernel" in names and "conv3x3_split_tail_colour_kernel" not in names
    assert torch.isfinite(raw2).all()
    pipe.close()
    ops.range_reset()


@pytest.mark.parametrize("mode", ["zero", "input"])
def test_pipeline_runs_colour_models_fused_and_unfused(mode):
    """A real renderer, a few frames with the next frame prefetched: ``fused=True`` (HIP assembly + colour tail) against
    ``fused=False`` (``LoadedModel.inference`` + clamp) at the tolerance of
    test_tail_gpu.py::test_pipeline_uses_the_fused_tail_and_matches_the_unfused_frame; ``previous`` has three channels; ``graph=True``
    silently runs eagerly."""
    from isosurfacesuperresolution_amd import models, ops, volumes as V
    from isosurfacesuperresolution_amd.inference import DirectRenderer, LoadedModel
    from isosurfacesuperresolution_amd.pipeline import SuperResolutionPipeline, default_shading
    torch.manual_seed(3)
    net = models.createNetwork('EnhanceNet', 4, 56, [0, 1, 2], 3, OPT)
    lm = LoadedModel.from_model(net, "cuda", parameters={"initialImage": mode})
    renderer = DirectRenderer()
    renderer.load_dense(V.ejecta(64))
    origins = [V.orbit_camera(k) for k in range(4)]
    frames = {}
    for fused in (True, False):
        pipe = SuperResolutionPipeline(renderer, lm, default_shading("cuda", 30.0), (96, 56), fused=fused, graph=True)
        assert pipe.colour and pipe.fused == fused and not pipe.graph
        pipe.set_static(fov=30.0, isovalue=0.34)
        pipe.frame(origins[0])
        pipe.reset()
        ops.profile_enable(True)
        out = []
        for k in range(3):
            rgb, raw = pipe.frame(origins[k], next_origin=origins[k + 1]) if fused else pipe.frame(origins[k])
            assert rgb.shape == (1, 3, 224, 384) and raw.shape == (1, 3, 224, 384)
            assert pipe.previous.shape[1] == 3 and pipe.previous.min() >= 0 and pipe.previous.max() <= 1
            out.append((rgb.clone(), raw.clone()))
        torch.cuda.synchronize()
        names = {n for n, _, _ in ops.profile_records()}
        ops.profile_enable(False)
        assert ("conv3x3_split_tail_colour_kernel" in names) == fused and ("conv3x3_small_cout_kernel" in names) == (not fused)
        assert not (names & UNSHADED_FRAME_KERNELS)
        assert pipe.graph_replays == 0
        pipe.close()
        frames[fused] = out
    for (rgb_a, raw_a), (rgb_b, raw_b) in zip(frames[True], frames[False]):
        assert torch.equal(rgb_a, raw_a) and torch.equal(rgb_b, raw_b)                 # one tensor: the displayed RGB is the next previous
        assert (raw_a - raw_b).abs().max().item() <= 1e-4
    assert (frames[True][0][1] - frames[False][0][1]).abs().max().item() <= 5e-5      # first frame: no recurrence yet
    assert (frames[True][2][1] - frames[True][0][1]).abs().max().item() > 1e-3        # (the frames do differ)
