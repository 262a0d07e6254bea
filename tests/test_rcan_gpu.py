"""GPU: the RCAN generator on the HIP kernels -- the module on the device against frames of the reference itself
(tests/golden/make_rcan_fixtures.py), the fused colour frame (``pipeline.run_network_colour``, ``SuperResolutionPipeline``), other
sizes against the CPU in fp64, gradients, and a row of the colour statistics table."""
import copy
import os
import warnings

import numpy as np
import pytest
import torch

from rcan_common import BOUND, G, PREMISE, rcan_net, small_rcan

pytestmark = pytest.mark.gpu

POOL, GATE, TAIL = "channel_pool_kernel", "gate_scale_add_kernel", "shuffle_tail_kernel"


def _profiled(fn):
    from isosurfacesuperresolution_amd import ops
    ops.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        names = [n for n, _, _ in ops.profile_records()]
    finally:
        ops.profile_enable(False)
    return out, names


@pytest.fixture(scope="module")
def net_a():
    return rcan_net("a").cuda()


@pytest.mark.parametrize("case", ["a", "b"])
def test_module_on_the_device_matches_the_reference(case, net_a):
    """Every stored frame single-step from the stored network input: prediction and the tensor after ``net.rir`` <= 1e-4, on the premise
    -- recorded in the fixture for both -- that the reference's fp32 is within 4e-5 of fp64; the frame-0 gates <= 1e-5.  Every block's
    attention is two launches, the tail one; the network's layers fit the range guard's words and nothing is hot."""
    from isosurfacesuperresolution_amd import ops
    assert max(G[case + "_cpu32_vs_fp64_single_step"].max(), G[case + "_rir_cpu32_vs_fp64_single_step"].max()) <= PREMISE
    ops.range_reset()
    net = net_a if case == "a" else rcan_net(case).cuda()
    post = net.net['post']
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)                    # no PyTorch-route warning: every layer on a kernel of the package
        for k in range(G[case + "_input"].shape[0]):
            x = torch.from_numpy(G[case + "_input"][k:k + 1]).cuda()
            gates = []
            (pred, residual), names = _profiled(lambda: net(x))
            rir = net.forward_features(x, gates=gates)
            assert (names.count(POOL), names.count(GATE), names.count(TAIL)) == (200, 200, 1), names
            assert torch.equal(pred, ops.pixel_shuffle4_conv(rir, post.weight, post.bias, clamp=True))
            err = np.abs(pred.cpu().numpy()[0] - G[case + "_prediction"][k]).max()
            err_rir = np.abs(rir.cpu().numpy()[0] - G[case + "_rir"][k]).max()
            print("rcan %s frame %d: prediction %.3g, rir %.3g (rir max %.3g)" % (case, k, err, err_rir, np.abs(G[case + "_rir"][k]).max()))
            assert err <= BOUND and err_rir <= BOUND, (case, k, err, err_rir)
            assert residual.shape == (1, 3, 32, 48)
            if k == 0:
                err_g = np.abs(torch.cat(gates).cpu().numpy() - G[case + "_gates_frame0"]).max()
                print("rcan %s frame 0: gates %.3g" % (case, err_g))
                assert err_g <= 1e-5
    st = ops._range_state("cuda")
    assert len(st["slots"]) <= 414                                       # one word per convolution; the gate launches share their block's
    assert not ops.refresh_range_flags("cuda") and not ops.any_hot("cuda")


def test_run_network_colour_equals_the_module_bit_for_bit(net_a):
    """The fused route runs the same launches as ``model(x)[0]``, its clamp in the tail's epilogue; ``LoadedModel.inference`` from the
    rendered channels gives the stored frame."""
    from isosurfacesuperresolution_amd import ops
    from isosurfacesuperresolution_amd.inference import LoadedModel
    from isosurfacesuperresolution_amd.pipeline import fused_path_ok, run_network_colour
    from rcan_common import SEQ
    lm = LoadedModel.from_model(net_a, "cuda")
    assert fused_path_ok(lm) and not lm.unshaded and lm.input_channels == 56 and lm.has_normal and lm.has_depth
    called = []
    with torch.no_grad():
        for k in (0, 3):
            x = torch.from_numpy(G["a_input"][k:k + 1]).cuda()
            frame = run_network_colour(lm, x, after_trunk=lambda: called.append(k))
            module = lm.model(x)[0]
            assert frame.shape == (1, 3, 32, 48) and torch.equal(frame, module)
            assert np.abs(frame.cpu().numpy()[0] - G["a_prediction"][k]).max() <= BOUND
        low = torch.from_numpy(SEQ["low"][0:1]).cuda()
        out = lm.inference(low, None)
        assert np.abs(out.cpu().numpy()[0] - G["a_prediction"][0]).max() <= BOUND
    assert called == [0, 3]
    ops.guards_flush("cuda")


def test_pipeline_with_a_colour_rcan_is_fused():
    """``SuperResolutionPipeline`` with an RCAN of 2 x 2 blocks on a small render takes the fused route: three recurrent frames."""
    import render_scenes
    from isosurfacesuperresolution_amd import volumes as V
    from isosurfacesuperresolution_amd.inference import DirectRenderer, LoadedModel
    from isosurfacesuperresolution_amd.pipeline import SuperResolutionPipeline, default_shading
    renderer = DirectRenderer()
    renderer.load_dense(render_scenes.scene_a()[0])
    lm = LoadedModel.from_model(small_rcan(2, 2), "cuda")
    pipe = SuperResolutionPipeline(renderer, lm, default_shading("cuda", 45.0), (48, 32))
    pipe.set_static(fov=45.0, isovalue=0.5)
    assert pipe.fused and pipe.colour and not pipe.graph
    frames = []
    for k in range(3):
        (rgb, raw), names = _profiled(lambda: pipe.frame(V.orbit_camera(k), next_origin=V.orbit_camera(k + 1)))
        assert (names.count(POOL), names.count(GATE), names.count(TAIL)) == (4, 4, 1), names
        assert rgb.shape == (1, 3, 128, 192) and torch.equal(rgb, raw) and pipe.previous is raw
        assert rgb.min().item() >= 0 and rgb.max().item() <= 1 and torch.isfinite(rgb).all()
        frames.append(rgb.clone())
    assert (pipe.gbuffer[..., 3] != 0).any()                       # the scene is in view: the frame is not a frame of background
    assert not torch.equal(frames[1], frames[2])
    pipe.close()
    # the module route (fused=False) from the same camera gives the first frame
    pipe2 = SuperResolutionPipeline(renderer, lm, default_shading("cuda", 45.0), (48, 32), fused=False)
    pipe2.set_static(fov=45.0, isovalue=0.5)
    rgb2, _ = pipe2.frame(V.orbit_camera(0))
    assert (rgb2 - frames[0]).abs().max().item() <= BOUND
    pipe2.close()


def test_small_network_at_an_odd_size_against_fp64():
    """2 x 2 blocks at 37 x 53 (several tiles of every kernel, no dimension a multiple of four): <= 1e-4 of the CPU in fp64."""
    from isosurfacesuperresolution_amd import ops
    ops.range_reset()
    net = small_rcan(2, 2)
    ref = copy.deepcopy(net).double()
    x = torch.rand(1, 56, 37, 53, generator=torch.Generator().manual_seed(8))
    with torch.no_grad():
        want, want_res = ref(x.double())
        net = net.cuda()
        got, got_res = net(x.cuda())
    err, err_res = (got.double().cpu() - want).abs().max().item(), (got_res.double().cpu() - want_res).abs().max().item()
    print("rcan 2x2 at 37x53 against fp64: prediction %.3g, second output %.3g" % (err, err_res))
    assert got.shape == (1, 3, 148, 212) and err <= BOUND and err_res <= BOUND
    ops.range_reset()


def test_gradients_against_fp64_on_the_cpu():
    """1 x 2 blocks at 8 x 12: loss and every parameter's gradient against CPU fp64 autograd, as per-parameter relative-norm errors:
    max <= 1e-2, median <= 1e-3, loss <= 1e-5 relative (the bounds of tests/test_tecogan_train_gpu.py for its clip gradients).  Under
    autograd the convolutions run on the HIP training kernels, the attention and the tail on the torch composite."""
    from isosurfacesuperresolution_amd import train
    g = torch.Generator().manual_seed(4)
    x, target = torch.rand(2, 56, 8, 12, generator=g), torch.rand(2, 3, 32, 48, generator=g)

    def loss_of(net, x, target):
        pred, residual = net(x)
        return ((pred - target) ** 2).mean() + 0.1 * (residual ** 2).mean()
    net = small_rcan(1, 2).train()
    ref = copy.deepcopy(net).double()
    ref_loss = loss_of(ref, x.double(), target.double())
    ref_loss.backward()
    net = net.cuda()
    loss = loss_of(net, x.cuda(), target.cuda())
    train.backward(loss)
    assert abs(loss.item() - ref_loss.item()) <= 1e-5 * max(1.0, abs(ref_loss.item()))
    errs = {}
    for (name, p), r in zip(net.named_parameters(), ref.parameters()):
        assert p.grad is not None and p.grad.shape == p.shape and r.grad.norm().item() > 0, name
        errs[name] = ((p.grad.cpu().double() - r.grad).norm() / r.grad.norm()).item()
    ranked = sorted(errs.items(), key=lambda kv: kv[1])
    print("RCAN gradients vs fp64: max %.3g (%s), median %.3g" % (ranked[-1][1], ranked[-1][0], ranked[len(ranked) // 2][1]))
    assert ranked[-1][1] <= 1e-2, ranked[-4:]
    assert ranked[len(ranked) // 2][1] <= 1e-3, ranked[-8:]


def test_colour_statistics_row_of_an_rcan_equals_the_cpu_table(tmp_path):
    """One clip through ``stats.run_colour_statistics`` (the model goes through ``guarded_forward``): the row of the run on the device
    against the row of the CPU run, at the tolerances of tests/test_metrics_gpu.py (PSNR 1e-3 dB, MS-SSIM 1e-5)."""
    from isosurfacesuperresolution_amd import inference, ops, stats, volumes as V
    from isosurfacesuperresolution_amd.dataset_video import render_clip
    r = inference.DirectRenderer()
    r.load_dense(V.ejecta(128))
    folder = tmp_path / "clips"
    folder.mkdir()
    origins = [V.orbit_camera(k, K=64, distance=1.9, pitch=0.3) for k in range(3)]
    high, low, flow = render_clip(r, origins, (128, 72), isovalue=0.34, ao_samples=4, ao_radius=0.05)
    for name, arr in (("high", high), ("low", low), ("flow", flow)):
        np.save(folder / ("%s_%05d.npy" % (name, 0)), arr)
    state = small_rcan(2, 2).state_dict()

    def specs():
        from isosurfacesuperresolution_amd import models
        return [{"name": "rcan", "model": models.RCAN.from_state_dict(state, [0, 1, 2])}]
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    rows = {}
    for dev in ("cuda", "cpu"):
        res = stats.run_colour_statistics([("Ejecta", [str(folder)])], specs(), str(tmp_path / dev), device=dev, log=lambda *a: None)
        lines = open(os.path.join(str(tmp_path / dev), "Stats_Ejecta_rcan.txt")).read().splitlines()
        assert lines[0] == "PSNR-color\tSSIM-color" and len(lines) == 2
        rows[dev] = np.array([float(v) for v in lines[1].split("\t")])
        assert res["Ejecta"]["rcan"]["PSNR-color"][2] == 1
        if dev == "cuda":
            assert not ops.any_hot("cuda")
    print("rcan colour row: device", rows["cuda"].tolist(), "cpu", rows["cpu"].tolist())
    assert np.isfinite(rows["cuda"]).all() and np.isfinite(rows["cpu"]).all()
    assert abs(rows["cuda"][0] - rows["cpu"][0]) <= 1e-3 and abs(rows["cuda"][1] - rows["cpu"][1]) <= 1e-5, rows
    ops.range_reset()
