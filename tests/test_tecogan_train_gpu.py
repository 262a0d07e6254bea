"""GPU: TRAINING a TecoGAN on the HIP path -- ``train.clip_loss`` / ``train.backward`` / ``train.GraphedTrainStep`` as they stand, the
two learned x2 upsamplings on the transposed convolution's own backward kernels (tests/test_convt_train_gpu.py).

A direct (reconType 'direct') unshaded 101 -> 6 TecoGAN with 2 residual layers, B = 2 clips of T = 3 frames, 8 x 8 -> 32 x 32 crops,
the loss recipe of the README / bench.py."""
import argparse
import copy
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

RECIPE = "l1:mask:1,l1:ao:1,l1:normal:10,l1:depth:10,temp-l2:color:0.1"
OPT = argparse.Namespace(upsample='bilinear', reconType='direct', useBN=False, numResidualLayers=2, losses=RECIPE,
                         lossAO=0.0, lossAmbient=0.1, lossDiffuse=0.9, lossSpecular=0.0)
B, T, LOW, HIGH, PAD = 2, 3, 8, 32, 4


def _clip(seed):
    g = torch.Generator().manual_seed(seed)
    inp = torch.rand(B, T, 5, LOW, LOW, generator=g); inp[:, :, 0] = inp[:, :, 0] * 2 - 1
    flow = (torch.rand(B, T, 2, LOW, LOW, generator=g) - 0.5) * 0.05
    tgt = torch.rand(B, T, 6, HIGH, HIGH, generator=g); tgt[:, :, 0] = tgt[:, :, 0] * 2 - 1
    return inp, flow, tgt


def _net(seed=124):
    from isosurfacesuperresolution_amd import models
    torch.manual_seed(seed)
    return models.createNetwork('TecoGAN', 4, 101, [0, 1, 2, 3, 4], 6, OPT)


def _crit(device):
    from isosurfacesuperresolution_amd import losses as L
    return L.LossNetUnshaded(device, 5, 6, HIGH, PAD, OPT).to(device)


def test_clip_gradients_on_the_hip_path_match_fp64_on_the_cpu():
    """Loss and every parameter's gradient of a clip (recurrence, backward through time, deferred weight gradients) against the same
    clip on the CPU in fp64, as per-parameter relative-norm errors: max <= 1e-2, median <= 1e-3, loss <= 1e-5 relative -- the bounds
    of test_clip_gradients_with_fused_kernels_match_module_path (a LeakyReLU input within rounding of zero moves a gradient by
    O(1e-4) in relative L2)."""
    from isosurfacesuperresolution_amd import train
    batch = _clip(3)
    net = _net()
    ref_net = copy.deepcopy(net).double()
    ref_loss, ref_sum = train.clip_loss(ref_net, _crit("cpu").double(), *(t.double() for t in batch), initial_image="zero")
    ref_loss.backward()
    net = net.cuda()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)                    # no PyTorch-route warning: every layer on a kernel of the package
        loss, loss_sum = train.clip_loss(net, _crit("cuda"), *(t.cuda() for t in batch), initial_image="zero")
        train.backward(loss)
    assert abs(loss_sum.item() - ref_sum.item()) <= 1e-5 * max(1.0, abs(ref_sum.item()))
    errs = {}
    for (name, p), r in zip(net.named_parameters(), ref_net.parameters()):
        assert p.grad is not None and p.grad.shape == p.shape, name
        errs[name] = ((p.grad.cpu().double() - r.grad).norm() / r.grad.norm()).item()
    ranked = sorted(errs.items(), key=lambda kv: kv[1])
    print("TecoGAN clip gradients vs fp64: max %.3g (%s), median %.3g" % (ranked[-1][1], ranked[-1][0], ranked[len(ranked) // 2][1]))
    assert ranked[-1][1] <= 1e-2, ranked[-4:]
    assert ranked[len(ranked) // 2][1] <= 1e-3, ranked[-8:]


def test_graphed_train_step_reproduces_the_eager_step_on_every_replay():
    """``train.GraphedTrainStep`` takes a TecoGAN as it stands: replay k leaves the gradients and the loss of eager step k (relative
    norm <= 1e-3, loss <= 1e-5 relative: the bounds of test_clip_gradients_inside_a_hip_graph_are_reproduced_by_every_replay) -- the
    weight images of the transposed convolutions are refreshed inside the graph after every captured optimizer step."""
    from isosurfacesuperresolution_amd import train
    batch = tuple(t.cuda() for t in _clip(5))
    crit = _crit("cuda")
    eager_net, graph_net = _net(11).cuda(), _net(11).cuda()
    # (flat Adam, as bench.py --mode train: every gradient is a view of one bucket that the graph writes, so a replay's gradients can be read)
    eager_opt, _ = train.make_optimizer(eager_net, lr=1e-4, capturable=True, flat=True)
    graph_opt, _ = train.make_optimizer(graph_net, lr=1e-4, capturable=True, flat=True)
    step = train.GraphedTrainStep(graph_net, crit, graph_opt, batch, warmup=3, initial_image="zero")
    for k in range(3):
        eager_opt.zero_grad()
        loss, loss_sum = train.clip_loss(eager_net, crit, *batch, initial_image="zero")
        train.backward(loss)
        eager_loss = loss_sum.item() / T
        grads = [p.grad.detach().clone() for p in eager_net.parameters()]
        eager_opt.step()
        graph_loss = float(step(batch))
        torch.cuda.synchronize()
        assert abs(graph_loss - eager_loss) <= 1e-5 * max(1.0, abs(eager_loss)), (k, graph_loss, eager_loss)
        for (name, p), r in zip(graph_net.named_parameters(), grads):
            assert ((p.grad - r).norm() / r.norm()).item() <= 1e-3, (k, name)


def test_twenty_steps_on_one_clip_lower_the_loss():
    from isosurfacesuperresolution_amd import train
    batch = tuple(t.cuda() for t in _clip(7))
    net, crit = _net(3).cuda(), _crit("cuda")
    optim, _ = train.make_optimizer(net, lr=1e-4)
    history = [train.train_step(net, crit, optim, batch, initial_image="zero") for _ in range(20)]
    assert all(torch.isfinite(p).all() for p in net.parameters())
    assert history[-1] < history[0], history
