"""GPU: the batch-norm EnhanceNet (``useBN``) at model level, at 8 x 12 / 8 x 8 only.  Eval mode: the batch-norm layers folded into
their convolutions (``ops.fold_batch_norm``) -- the network IS a plain EnhanceNet: the same kernels, the same bits, every fused route,
against the reference fixture (tests/golden/bn_reference.npz).  Train mode: ``ops.batch_norm`` on the kernels of
csrc/sr_batchnorm.hip, against the fixture's fp64 step, eagerly and inside ``train.GraphedTrainStep``."""
import argparse
import warnings

import pytest
import torch
import torch.nn.functional as F

from bn_common import BOUND, G, PREMISE, bn_net, check_train_case, folded_plain_net, train_batch, train_case
from train_route_common import observed

from isosurfacesuperresolution_amd import ops

pytestmark = pytest.mark.gpu

BN_KERNELS = {"batch_norm_stat_kernel", "batch_norm_finish_kernel", "batch_norm_apply_kernel",
              "batch_norm_grad_sum_kernel", "batch_norm_grad_finish_kernel", "batch_norm_backward_kernel"}


def _planes(x):
    """The tensor as the frame pipeline's input assembly leaves it (``ops.empty_planes``), on the device."""
    out = ops.empty_planes(*x.shape, "cuda")
    out.copy_(x)
    return out


def _loaded(net):
    from isosurfacesuperresolution_amd.inference import LoadedModel
    return LoadedModel.from_model(net, "cuda")


def _module_composition(net, x):
    """The network as ``nn.Sequential`` would run it (conv, BatchNorm2d, ReLU, ... on PyTorch's operators)."""
    f = net.preblock(x)
    for block in net.blocks:
        f = f + block(f)
    return net._recon_image(x, net.postblock(f))[0]


def test_case_a_unshaded_eval_frame_matches_the_reference():
    assert float(G["a_cpu32_vs_fp64"].max()) <= PREMISE
    net = bn_net("a").cuda()
    x = _planes(torch.from_numpy(G["a_input"][0:1]))
    with torch.no_grad():
        (pred, _), _, names = observed(lambda: net(x))
    err = (pred.cpu() - torch.from_numpy(G["a_prediction"][0:1])).abs().max().item()
    print("case a: %.3e; kernels %s" % (err, sorted(set(names))))
    assert err <= BOUND
    assert not (set(names) & BN_KERNELS)
    assert not ops.any_hot(pred.device)


def test_case_b_colour_eval_frames_match_the_reference():
    from isosurfacesuperresolution_amd.pipeline import fused_path_ok, run_network_colour
    assert float(G["b_cpu32_vs_fp64"].max()) <= PREMISE
    lm = _loaded(bn_net("b"))
    assert fused_path_ok(lm)                             # a colour batch-norm model takes the fused frame path now
    with torch.no_grad():
        for k in range(G["b_input"].shape[0]):
            x = _planes(torch.from_numpy(G["b_input"][k:k + 1]))
            frame, _, names = observed(lambda: run_network_colour(lm, x))
            pred, _ = lm.model(x)
            ref = torch.from_numpy(G["b_prediction"][k:k + 1])
            err_frame = (frame.cpu() - ref.clamp(0, 1)).abs().max().item()
            err_module = (pred.cpu() - ref).abs().max().item()
            print("case b frame %d: fused frame %.3e, module route %.3e" % (k, err_frame, err_module))
            assert err_frame <= BOUND and err_module <= BOUND
            assert "conv3x3_split_tail_colour_kernel" in names and not (set(names) & BN_KERNELS)
    assert not ops.any_hot(frame.device)


@pytest.mark.parametrize("case", ["a", "b"])
def test_folded_net_is_the_plain_net_bit_for_bit(case):
    """The eval-mode batch-norm net and a plain net that carries ``ops.fold_batch_norm``'s tensors: ``torch.equal`` outputs and the SAME
    list of kernel names, through the module route and through ``run_network`` / ``run_network_colour``."""
    from isosurfacesuperresolution_amd.pipeline import default_shading, run_network, run_network_colour
    net = bn_net(case).cuda()
    plain = folded_plain_net(net)
    x = torch.from_numpy(G[case + "_input"][0:1])
    with torch.no_grad():
        (got, _), _, names = observed(lambda: net(_planes(x)))
        (want, _), _, names_plain = observed(lambda: plain(_planes(x)))
        assert torch.equal(got, want) and names == names_plain and names
        lm, lm_plain = _loaded(net), _loaded(plain)
        if case == "a":
            shading = default_shading("cuda", 45.0)
            run = lambda m: run_network(m, shading, _planes(x))
        else:
            run = lambda m: (run_network_colour(m, _planes(x)),)
        run(lm); run(lm_plain)                           # (weight images prepared)
        outs, _, names = observed(lambda: run(lm))
        outs_plain, _, names_plain = observed(lambda: run(lm_plain))
    assert names == names_plain and names
    for a, b in zip(outs, outs_plain):
        assert torch.equal(a, b)
    assert not ops.any_hot(got.device)


def test_pipeline_renders_an_unshaded_batch_norm_model_fused():
    """``SuperResolutionPipeline(fused=True)`` with an unshaded ``useBN`` model: two frames on the fused path (the dataflow trunk on
    the folded convolutions); the frame graph stays off."""
    from isosurfacesuperresolution_amd import volumes as V
    from isosurfacesuperresolution_amd.inference import DirectRenderer
    from isosurfacesuperresolution_amd.pipeline import SuperResolutionPipeline, default_shading
    renderer = DirectRenderer()
    renderer.load_dense(V.sphere64())
    pipe = SuperResolutionPipeline(renderer, _loaded(bn_net("a")), default_shading("cuda", 45.0), (64, 48), graph=True)
    assert pipe.fused and not pipe.graph
    pipe.set_static(fov=45.0, isovalue=0.5)
    names = []
    for k in (2, 3):
        (rgb, raw), _, n = observed(lambda: pipe.frame(V.quantize3(V.orbit_camera(k))))
        names += n
        assert rgb.shape == (1, 3, 192, 256) and raw.shape == (1, 6, 192, 256)
        assert torch.isfinite(rgb).all() and torch.isfinite(raw).all()
    assert not (set(names) & BN_KERNELS) and names
    pipe.close()


def test_case_t_train_mode_step_matches_the_reference_fp64(monkeypatch):
    """One train-mode call on the device against the fixture's fp64 step; 20 batch-norm layers on the new kernels and none on PyTorch's."""
    x, cot = train_batch()
    net = bn_net("t").cuda()

    def refuse(*a, **kw):
        raise AssertionError("PyTorch's batch norm ran inside the step")
    monkeypatch.setattr(F, "batch_norm", refuse)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)       # no PyTorch-route warning either
        res, _, names = observed(lambda: train_case(net, x.cuda(), cot.cuda()))
    assert names.count("batch_norm_stat_kernel") == 20 and names.count("batch_norm_apply_kernel") == 20
    assert names.count("batch_norm_grad_sum_kernel") == 20 and names.count("batch_norm_backward_kernel") == 20
    assert "trunk_dataflow_kernel" not in names and "conv3x3_split_block2_kernel" not in names
    check_train_case(res, pred_bar=BOUND, grad_bar=1e-4, stat_bar=1e-5)
    assert int(net.blocks[0][1].num_batches_tracked) == 1


RECIPE = "l1:mask:1,l1:ao:1,l1:normal:10,l1:depth:10,temp-l2:color:0.1"
OPT = argparse.Namespace(upsample='bilinear', reconType='residual', useBN=True, numResidualLayers=10, losses=RECIPE,
                         lossAO=0.0, lossAmbient=0.1, lossDiffuse=0.9, lossSpecular=0.0)
B, T, LOW, HIGH, PAD = 2, 3, 8, 32, 4


def _clip(seed):
    g = torch.Generator().manual_seed(seed)
    inp = torch.rand(B, T, 5, LOW, LOW, generator=g); inp[:, :, 0] = inp[:, :, 0] * 2 - 1
    flow = (torch.rand(B, T, 2, LOW, LOW, generator=g) - 0.5) * 0.05
    tgt = torch.rand(B, T, 6, HIGH, HIGH, generator=g); tgt[:, :, 0] = tgt[:, :, 0] * 2 - 1
    return inp, flow, tgt


def _train_net(seed):
    from isosurfacesuperresolution_amd import models
    torch.manual_seed(seed)
    return models.createNetwork('EnhanceNet', 4, 101, [0, 1, 2, 3, 4], 6, OPT).cuda().train()


def _fold64(weight, bias, bn):
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return weight.detach().double() * s[:, None, None, None], (bias.detach().double() - bn.running_mean.double()) * s + bn.bias.detach().double()


def test_train_step_eager_and_graphed_then_inference_with_the_new_statistics():
    """Three steps on one tiny batch, ``train.train_step`` eagerly and ``train.GraphedTrainStep``: the graphed losses equal the eager ones
    to 1e-5 relative and so do the running statistics after three replays (1e-5 of the activations' scale, see below); after ``model.eval()`` the next inference frame is made of the NEW statistics -- the fold was refreshed
    after replays that never advanced a version counter."""
    from isosurfacesuperresolution_amd import losses as L, train
    batch = tuple(t.cuda() for t in _clip(5))
    crit = L.LossNetUnshaded("cuda", 5, 6, HIGH, PAD, OPT).to("cuda")
    eager_net, graph_net = _train_net(11), _train_net(11)
    x = _planes(torch.from_numpy(G["a_input"][0:1]))
    with torch.no_grad():                                  # an inference frame BEFORE training: the fold of the initial statistics exists
        before, _ = graph_net.eval()(x)
        folded = [w for w, _ in graph_net.trunk_convs()[1:]]
        versions = [w._version for w in folded]
    graph_net.train()
    # Plain SGD, not Adam: the gradients of two runs of one step differ in their last bits (1.3e-7 of the largest, measured, with the
    # batch norm on PyTorch's operator as well), and Adam normalises a gradient that IS such noise -- the bias of a convolution in front
    # of a batch norm has a mathematically zero one -- to a step of +-lr, after which two runs' weights and running means are 1e-4
    # apart without a trace in the loss.  SGD keeps the noise the size it has, so that the comparison below is about the statistics.
    eager_opt, graph_opt = (torch.optim.SGD(net.parameters(), lr=1e-3) for net in (eager_net, graph_net))
    step = train.GraphedTrainStep(graph_net, crit, graph_opt, batch, warmup=3, initial_image="zero")
    assert int(graph_net.blocks[0][1].num_batches_tracked) == 0           # the warm-up steps were undone, buffers included
    for k in range(3):
        eager_loss = train.train_step(eager_net, crit, eager_opt, batch, initial_image="zero")
        graph_loss = float(step(batch))
        torch.cuda.synchronize()
        print("step %d: eager %.6f graphed %.6f" % (k, eager_loss, graph_loss))
        assert abs(graph_loss - eager_loss) <= 1e-5 * max(1.0, abs(eager_loss)), (k, graph_loss, eager_loss)
    assert int(graph_net.blocks[0][1].num_batches_tracked) == 3 * T == int(eager_net.blocks[0][1].num_batches_tracked)
    # The statistics are averages of activations, and the activations of the two runs agree as their losses do: 1e-5 of the activations'
    # SCALE -- a layer's sqrt(max running_var) for its mean (a mean near zero cannot be held relative to itself), max running_var for
    # its variance.
    worst = 0.0
    eager_buffers = dict(eager_net.named_buffers())
    for name, got in graph_net.named_buffers():
        if name.endswith("num_batches_tracked"):
            continue
        var = eager_buffers[name.rsplit(".", 1)[0] + ".running_var"].max().item()
        scale = var if name.endswith("running_var") else var ** 0.5
        err = (got - eager_buffers[name]).abs().max().item()
        worst = max(worst, err / scale)
        assert err <= 1e-5 * scale, (name, err, scale)
    print("running statistics, graphed against eager: worst %.3e of the activations' scale" % worst)
    assert not torch.equal(graph_net.blocks[0][1].running_mean, torch.zeros_like(graph_net.blocks[0][1].running_mean))
    graph_net.eval()
    with torch.no_grad():
        convs = graph_net.trunk_convs()[1:]
        assert all(w is f for (w, _), f in zip(convs, folded))                       # the persistent tensors, rewritten in place
        assert all(w._version > v for (w, _), v in zip(convs, versions))
        for block, pair in zip(graph_net.blocks, zip(convs[0::2], convs[1::2])):
            for i, (w, b) in zip((0, 3), pair):
                w64, b64 = _fold64(block[i].weight, block[i].bias, block[i + 1])
                assert (w.double() - w64).abs().max().item() <= 1e-6 * w64.abs().max().item()
                assert (b.double() - b64).abs().max().item() <= 1e-6 * max(1.0, b64.abs().max().item())
        after, _ = graph_net(x)
        ref = _module_composition(graph_net, x)
    err = (after - ref).abs().max().item()
    print("inference after three replays: %.3e from the module composition, %.3e from the frame before training"
          % (err, (after - before).abs().max().item()))
    assert err <= BOUND * max(1.0, ref.abs().max().item())
