"""The fp64 definitions the GPU tests of the training convolutions compare against (train_route_common.fwd64 / dgrad64) are the
operations autograd differentiates: a reference that had the taps or the channel pair the wrong way round would make every kernel
test behind it assert the wrong thing.  Odd sizes and unequal channel counts, so that a transposition or a flip cannot cancel."""
import pytest
import torch
import torch.nn.functional as F

from train_route_common import dgrad64, fwd64

SHAPES = [(2, 5, 7, 6, 9), (1, 101, 64, 5, 4), (3, 64, 6, 3, 8), (1, 3, 3, 1, 1)]      # N, Cin, Cout, H, W


def _operands(shape, seed):
    n, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, cin, h, w, generator=g, dtype=torch.float64) * 2 - 1).requires_grad_()
    wt = (torch.rand(cout, cin, 3, 3, generator=g, dtype=torch.float64) * 2 - 1) / (3.0 * cin ** 0.5)
    b = torch.rand(cout, generator=g, dtype=torch.float64) - 0.5
    gy = torch.rand(n, cout, h, w, generator=g, dtype=torch.float64) * 2 - 1
    return x, wt, b, gy


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_definition_is_conv2d_with_the_epilogues(shape):
    x, wt, b, _ = _operands(shape, 1)
    res = torch.randn(shape[0], shape[2], shape[3], shape[4], dtype=torch.float64)
    z = F.conv2d(x.detach(), wt, b, padding=1)
    assert torch.equal(fwd64(x.detach(), wt, b, 'relu', None), z.clamp(min=0))
    assert torch.equal(fwd64(x.detach(), wt, b, 'none', res), z + res)
    assert torch.equal(fwd64(x.detach().float(), wt.float(), None, 'none', None), F.conv2d(x.detach().float().double(), wt.float().double(), padding=1))


@pytest.mark.parametrize("shape", SHAPES)
def test_data_gradient_definition_is_autograds_input_gradient(shape):
    x, wt, b, gy = _operands(shape, 2)
    F.conv2d(x, wt, b, padding=1).backward(gy)
    ref = x.grad
    assert ref.abs().max().item() > 0
    assert (dgrad64(gy, wt) - ref).abs().max().item() <= 1e-13 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("shape", SHAPES[:3])
def test_gated_data_gradient_is_the_gradient_through_relu(shape):
    """t = relu(u); y = conv(t): dL/du = (t > 0) * dgrad(gy) -- the gate operand is the ReLU's OUTPUT, with exact zeros where it closed."""
    x, wt, b, gy = _operands(shape, 3)
    t = torch.relu(x)
    F.conv2d(t, wt, b, padding=1).backward(gy)
    ref = x.grad
    closed = t.detach() <= 0
    assert closed.any() and not closed.all()
    got = dgrad64(gy, wt, gate=t.detach())
    assert (got - ref).abs().max().item() <= 1e-13 * max(1.0, ref.abs().max().item())
    assert got[closed].abs().max().item() == 0.0
    assert (dgrad64(gy, wt)[closed] != 0).any()           # ... where the ungated gradient is not zero: the gate decides something


@pytest.mark.parametrize("shape", [(2, 6, 6, 5, 7), (1, 64, 64, 3, 4)])
def test_residual_block_gradient_is_two_data_gradients_with_gate_and_skip(shape):
    """y = x + conv2(relu(conv1(x))): dL/dx = dgrad(dgrad(gy, w2, gate = t), w1, skip = gy) with t the ReLU's output."""
    n, c, _, h, w = shape
    x, w1, b1, gy = _operands(shape, 4)
    _, w2, b2, _ = _operands(shape, 5)
    t = torch.relu(F.conv2d(x, w1, b1, padding=1))
    y = x + F.conv2d(t, w2, b2, padding=1)
    y.backward(gy)
    assert torch.equal(y.detach(), fwd64(fwd64(x.detach(), w1, b1, 'relu', None), w2, b2, 'none', x.detach()))
    gz = dgrad64(gy, w2, gate=t.detach())
    gx = dgrad64(gz, w1, skip=gy)
    assert (gx - x.grad).abs().max().item() <= 1e-13 * max(1.0, x.grad.abs().max().item())
