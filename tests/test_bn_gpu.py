"""The training-mode batch-norm kernels (csrc/sr_batchnorm.hip) through ``ops.batch_norm``, one launch group at a time against fp64
torch on the CPU.  Bars (tests/bn_common.py), none taken from the code under test: y and dx 2e-6 of max|ref| (the project's bar for
values and data gradients at K <= 576), dgamma and dbeta 1e-5 of max|ref| (its parameter-gradient bar), running statistics 1e-6
relative; PyTorch's own fp32 CPU batch norm stays inside all of them on exactly these inputs (worst: y 3.2e-7, dx 2.1e-7, dgamma
7.6e-7, dbeta 1.0e-6, running statistics 7.4e-8).  No M = 2 case: the fp32 reference itself is 1.6e-4 off there."""
import functools
import warnings

import pytest
import torch

from bn_common import KERNEL_SHAPES, PARAM_BAR, STAT_BAR, Y_BAR, kernel_inputs, make_bn, reference64, relerr
from train_route_common import observed

from isosurfacesuperresolution_amd import ops

pytestmark = pytest.mark.gpu

FORWARD = ["batch_norm_stat_kernel", "batch_norm_finish_kernel", "batch_norm_apply_kernel"]
BACKWARD = ["batch_norm_grad_sum_kernel", "batch_norm_grad_finish_kernel", "batch_norm_backward_kernel"]
FORMS = ["relu", "skip"]


@functools.lru_cache(maxsize=None)
def _case(shape, form):
    """(inputs on the CPU, fp64 reference): computed once per case and shared, never modified."""
    t = kernel_inputs(shape, seed=KERNEL_SHAPES.index(shape))
    return t, reference64(t, form)


def _call(t, form, bn, x, res):
    if form == "relu":
        return ops.batch_norm(x, bn, act='relu')
    return ops.batch_norm(x, bn, residual=res)


def _forward(t, form, grad):
    """One call on the device -> (bn, x, residual, y)."""
    bn = make_bn(t, "cuda")
    x = t["x"].cuda().requires_grad_(grad)
    res = t["residual"].cuda().requires_grad_(grad) if form == "skip" else None
    bn.weight.requires_grad_(grad); bn.bias.requires_grad_(grad)
    return bn, x, res, _call(t, form, bn, x, res)


def _check_forward(ref, bn, y, tag):
    figures = dict(y=relerr(y, ref["y"]), running_mean=relerr(bn.running_mean, ref["running_mean"]),
                   running_var=relerr(bn.running_var, ref["running_var"]))
    print(tag, " ".join("%s %.2e" % kv for kv in figures.items()))
    assert figures["y"] <= Y_BAR
    assert figures["running_mean"] <= STAT_BAR and figures["running_var"] <= STAT_BAR
    assert int(bn.num_batches_tracked) == 1


def _check_backward(ref, bn, x, res, dy, tag):
    figures = dict(dx=relerr(x.grad, ref["dx"]), dgamma=relerr(bn.weight.grad, ref["dgamma"]), dbeta=relerr(bn.bias.grad, ref["dbeta"]))
    print(tag, " ".join("%s %.2e" % kv for kv in figures.items()))
    assert figures["dx"] <= Y_BAR
    assert figures["dgamma"] <= PARAM_BAR and figures["dbeta"] <= PARAM_BAR
    if res is not None:
        assert torch.equal(res.grad, dy)             # the skip's gradient IS dy


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_launch_group(shape, form):
    t, ref = _case(shape, form)
    assert ops.batch_norm_supported(t["x"].cuda(), make_bn(t, "cuda"))
    with torch.no_grad():
        (bn, _, _, y), _, names = observed(lambda: _forward(t, form, False))
        assert names == FORWARD
        _check_forward(ref, bn, y, "forward %s %s:" % (shape, form))
        bn2, _, _, y2 = _forward(t, form, False)
    assert torch.equal(y2, y) and torch.equal(bn2.running_mean, bn.running_mean) and torch.equal(bn2.running_var, bn.running_var)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_autograd_node(shape, form):
    """Forward + backward as one node: the forward has the bits of the no-grad pieces, the backward is three launches."""
    t, ref = _case(shape, form)
    dy = t["dy"].cuda()
    with torch.no_grad():
        _, _, _, y_pieces = _forward(t, form, False)
    (bn, x, res, y), _, names = observed(lambda: _forward(t, form, True))
    assert names == FORWARD
    assert torch.equal(y, y_pieces)
    _check_forward(ref, bn, y, "node forward %s %s:" % (shape, form))
    _, _, names = observed(lambda: y.backward(dy))
    assert names == BACKWARD
    _check_backward(ref, bn, x, res, dy, "node backward %s %s:" % (shape, form))
    bn2, x2, res2, y2 = _forward(t, form, True)
    y2.backward(dy)
    assert torch.equal(x2.grad, x.grad) and torch.equal(bn2.weight.grad, bn.weight.grad) and torch.equal(bn2.bias.grad, bn.bias.grad)


def test_backward_launches_only_what_is_needed():
    t, ref = _case((2, 16, 4, 4), "relu")
    bn = make_bn(t, "cuda")
    x = t["x"].cuda()                                  # no gradient for x: the streaming pass is not launched
    y = ops.batch_norm(x, bn, act='relu')
    _, _, names = observed(lambda: y.backward(t["dy"].cuda()))
    assert names == BACKWARD[:2]
    assert relerr(bn.weight.grad, ref["dgamma"]) <= PARAM_BAR and relerr(bn.bias.grad, ref["dbeta"]) <= PARAM_BAR


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", [(3, 64, 5, 37), (16, 64, 32, 32)], ids=lambda s: "x".join(map(str, s)))
def test_switch_back_to_the_torch_operator(shape, form, monkeypatch):
    t, ref = _case(shape, form)
    monkeypatch.setattr(ops, "BATCH_NORM_KERNELS", False)
    dy = t["dy"].cuda()
    (bn, x, res, y), _, names = observed(lambda: _forward(t, form, True))
    assert not ops.batch_norm_supported(x, bn)
    _, _, names_b = observed(lambda: y.backward(dy))
    assert not [n for n in names + names_b if n.startswith("batch_norm")]
    _check_forward(ref, bn, y, "torch forward %s %s:" % (shape, form))
    _check_backward(ref, bn, x, res, dy, "torch backward %s %s:" % (shape, form))


@pytest.mark.parametrize("kw", [dict(momentum=None), dict(affine=False), dict(track_running_stats=False)])
def test_device_fall_backs_equal_f_batch_norm(kw):
    t, _ = _case((2, 16, 4, 4), "relu")
    ours, theirs = torch.nn.BatchNorm2d(16, **kw).cuda().train(), torch.nn.BatchNorm2d(16, **kw).cuda().train()
    x = t["x"].cuda()
    assert not ops.batch_norm_supported(x, ours)
    with warnings.catch_warnings():                    # (the route says so once per process: RuntimeWarning)
        warnings.simplefilter("ignore")
        got, _, names = observed(lambda: ops.batch_norm(x, ours, act='relu'))
    assert not [n for n in names if n.startswith("batch_norm")]
    with torch.backends.cudnn.flags(enabled=False):     # (the composition runs ATen's own kernels on the device)
        assert torch.equal(got, torch.relu(theirs(x)))


def test_one_value_per_channel_raises():
    bn = torch.nn.BatchNorm2d(4).cuda().train()
    with pytest.raises(ValueError):
        ops.batch_norm(torch.randn(1, 4, 1, 1, device="cuda"), bn)


@pytest.mark.parametrize("form", FORMS)
def test_forward_and_backward_are_capturable(form):
    """A ``torch.cuda.graph`` of forward + backward replayed twice advances the running statistics twice and equals two eager calls."""
    t, _ = _case((2, 16, 4, 4), form)
    dy = t["dy"].cuda()
    eager = []
    bn_e = make_bn(t, "cuda")
    for _ in range(2):
        x = t["x"].cuda().requires_grad_(True)
        res = t["residual"].cuda() if form == "skip" else None
        y = _call(t, form, bn_e, x, res)
        eager = [y.detach()] + list(torch.autograd.grad(y, (x, bn_e.weight, bn_e.bias), dy))

    bn_g = make_bn(t, "cuda")
    before = {k: v.clone() for k, v in bn_g.state_dict().items()}
    xs = t["x"].cuda().requires_grad_(True)
    res = t["residual"].cuda() if form == "skip" else None

    def step():
        y = _call(t, form, bn_g, xs, res)
        return [y.detach()] + list(torch.autograd.grad(y, (xs, bn_g.weight, bn_g.bias), dy))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.no_grad():
        for k, v in bn_g.state_dict().items():
            v.copy_(before[k])
    graph = torch.cuda.CUDAGraph()
    with ops.graph_capture(graph):
        outs = step()
    with torch.no_grad():                               # (a capture runs nothing, but the torch op on num_batches_tracked is recorded only)
        for k, v in bn_g.state_dict().items():
            v.copy_(before[k])
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bn_g.running_mean, bn_e.running_mean) and torch.equal(bn_g.running_var, bn_e.running_var)
    assert not torch.equal(bn_g.running_mean, before["running_mean"])
    assert int(bn_g.num_batches_tracked) == 2 == int(bn_e.num_batches_tracked)
    for got, want in zip(outs, eager):
        assert torch.equal(got, want)
