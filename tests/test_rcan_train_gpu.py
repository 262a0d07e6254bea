"""GPU: TRAINING an RCAN on the HIP path -- the backward kernels of csrc/sr_attention.hip behind ``ops.channel_attention_residual`` and
``ops.pixel_shuffle4_conv`` under autograd, and a colour clip through ``train.colour_clip_loss`` / ``train.backward`` /
``train.GraphedTrainStep``.

The reference throughout is CPU fp64 autograd of the ops' own definitions (``ops._channel_attention_cpu``,
``ops._pixel_shuffle4_conv_cpu``); the yardstick is the fp32 torch composite on the device (``ops.ATTENTION_KERNELS = False``) against
the same fp64: per gradient tensor the HIP path's relative L2 error must stay within max(2 x the composite's, 1e-6) -- the factor for
a different but legitimate summation order, the floor for a handful of fp32 roundings of 2^-24 each with x8 room."""
import copy
import warnings

import pytest
import torch

from rcan_common import small_rcan
from test_attention_gpu import SHAPES, _perceptron, _tensor

pytestmark = pytest.mark.gpu

FLOOR = 1e-6
# test_gate_and_scale_add's list ((2, 67, 129): two slabs and two chunks per plane) and a size that is no multiple of four
ATT_SHAPES = SHAPES + [(2, 37, 53)]
LAYOUTS = ["packed", "padded", "offset"]
ATT_NAMES = ("dx", "dt", "dWd", "dbd", "dWu", "dbu")
TAIL_NAMES = ("df", "dw", "db")
BACKWARD_KERNELS = ("gate_grad_sum_kernel", "gate_backward_kernel", "gate_param_grad_kernel", "shuffle_tail_dgrad_kernel",
                    "shuffle_tail_wgrad_kernel", "shuffle_tail_wgrad_sum_kernel")


def _laid_out(v, layout):
    """``v`` [n, 64, h, w] on the device: packed; with padded channel planes whose pad holds 1e30 (the 16-byte path with its per-element
    rest; ``_tensor``'s layout); or packed one float behind a 16-byte boundary (the per-element path)."""
    n, c, h, w = v.shape
    if layout == "packed":
        return v.cuda()
    if layout == "offset":
        buf = torch.full((v.numel() + 1,), 1e30, dtype=torch.float32, device="cuda")
        t = buf[1:].view(n, c, h, w)
    else:
        plane = h * w + (4 - h * w % 4) % 4 + 4
        buf = torch.full((n * c * plane,), 1e30, dtype=torch.float32, device="cuda")
        t = buf.as_strided((n, c, h, w), (c * plane, plane, w, 1))
    t.copy_(v)
    t._whole = buf
    return t


def _rel(got, want):
    want = want.double().cpu()
    return ((got.double().cpu() - want).norm() / want.norm().clamp_min(1e-300)).item()


def _attention_grads(operands, dy, kernels, slope=0.01):
    """Gradients of ``ops.channel_attention_residual`` for ``dy``, in the order of ATT_NAMES."""
    from isosurfacesuperresolution_amd import ops
    leaves = [v.detach().requires_grad_() for v in operands]
    before = ops.ATTENTION_KERNELS
    ops.ATTENTION_KERNELS = kernels
    try:
        y = ops.channel_attention_residual(*leaves, slope=slope)
        assert (type(y.grad_fn).__name__ == "_ChannelAttentionFunctionBackward") == (kernels and y.is_cuda)
        return y.detach(), torch.autograd.grad(y, leaves, dy)
    finally:
        ops.ATTENTION_KERNELS = before


def _tail_grads(f, wt, b, dout, kernels):
    from isosurfacesuperresolution_amd import ops
    leaves = [v.detach().requires_grad_() for v in (f, wt, b)]
    before = ops.ATTENTION_KERNELS
    ops.ATTENTION_KERNELS = kernels
    try:
        out = ops.pixel_shuffle4_conv(*leaves)
        assert (type(out.grad_fn).__name__ == "_PixelShuffle4ConvFunctionBackward") == (kernels and out.is_cuda)
        return out.detach(), torch.autograd.grad(out, leaves, dout)
    finally:
        ops.ATTENTION_KERNELS = before


def _judge(what, names, hip, composite, ref):
    worst = []
    for name, g, c, r in zip(names, hip, composite, ref):
        e_hip, e_comp = _rel(g, r), _rel(c, r)
        print("%s %s: HIP %.3g, composite %.3g" % (what, name, e_hip, e_comp))
        if e_hip > max(2 * e_comp, FLOOR):
            worst.append((name, e_hip, e_comp))
    assert not worst, (what, worst)


# ------------------------------------------------------------------------------------------------------------- attention backward

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,h,w", ATT_SHAPES)
def test_attention_backward_against_fp64(n, h, w, layout):
    """dx, dt and the four parameter gradients, per tensor, against CPU fp64 autograd of the definition; the forward under autograd has
    the bits of the no-grad call.  Measured columns: profiles/rcan_train.md (closest: 2 x 3 x 5, dWd 9.7e-07 against the floor of 1e-6
    -- du inherits the error of the forward gate's fp32 chain, and Wu^T du cancels over 64 channels)."""
    from isosurfacesuperresolution_amd import ops
    gen = torch.Generator().manual_seed(300 + h * w)
    x, t, dy = (_laid_out(torch.randn(n, 64, h, w, generator=gen), layout) for _ in range(3))
    t.add_(torch.randn(n, 64, 1, 1, generator=gen).cuda())          # per-channel means of order one: gates all over (0, 1)
    params = _perceptron(gen, scale=3.0)
    operands = (x, t) + params
    y, hip = _attention_grads(operands, dy, True)
    with torch.no_grad():
        assert torch.equal(y, ops.channel_attention_residual(*operands, slope=0.01))
    _, composite = _attention_grads(operands, dy, False)
    _, ref = _attention_grads([v.double().cpu() for v in operands], dy.double().cpu(), True)
    torch.cuda.synchronize()
    assert all(g.shape == r.shape and g.dtype == torch.float32 for g, r in zip(hip, ref))
    _judge("attention %dx%dx%d %s" % (n, h, w, layout), ATT_NAMES, hip, composite, ref)
    if layout != "packed":
        for v in (x, t, dy):
            assert (v._whole == 1e30).sum().item() == v._whole.numel() - v.numel()          # nothing wrote outside the tensors


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,h,w", [(2, 3, 5), (2, 37, 53), (2, 67, 129)])
def test_half_gate_is_exact(n, h, w, layout):
    """Wu = 0, bu = 0: the gate is exactly 0.5 and dz = 0, so dt is bitwise dy * 0.5 and dx bitwise dy on every alignment path; with
    small-integer dy and t every ds is exact, read through dbu = sum_n ds * 0.25."""
    gen = torch.Generator().manual_seed(17)
    x = _laid_out(torch.randn(n, 64, h, w, generator=gen), layout)
    t, dy = (_laid_out(torch.randint(-8, 9, (n, 64, h, w), generator=gen).float(), layout) for _ in range(2))
    wd, bd, _, _ = _perceptron(gen)
    operands = (x, t, wd, bd, torch.zeros(64, 4, device="cuda"), torch.zeros(64, device="cuda"))
    _, (dx, dt, dwd, dbd, dwu, dbu) = _attention_grads(operands, dy, True)
    assert torch.equal(dx, dy) and torch.equal(dt, dy * 0.5)
    ds = (dy.double() * t.double()).sum(dim=(2, 3))                   # |ds| <= 64 * 8643 < 2^24
    assert torch.equal(dbu.double(), (ds * 0.25).sum(dim=0))
    assert not dwd.any() and not dbd.any()                            # dg = Wu^T du = 0


# ------------------------------------------------------------------------------------------------------------------ tail backward

def _tail_case(n, h, w, cout, padded, seed, integers=False):
    gen = torch.Generator().manual_seed(seed)
    if integers:
        f = _tensor(gen, n, h, w, padded, integers=True)
        wt = torch.randint(-3, 4, (cout, 4, 3, 3), generator=gen).float().cuda()
        b = torch.randint(-5, 6, (cout,), generator=gen).float().cuda()
        dout = torch.randint(-3, 4, (n, cout, 4 * h, 4 * w), generator=gen).float().cuda()
    else:
        f = _tensor(gen, n, h, w, padded)
        wt = (torch.randn(cout, 4, 3, 3, generator=gen) * 0.3).cuda()
        b = (torch.randn(cout, generator=gen) * 0.5 + 0.5).cuda()
        dout = torch.randn(n, cout, 4 * h, 4 * w, generator=gen).cuda()
    return f, wt, b, dout


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("cout", [3, 5, 8])
@pytest.mark.parametrize("h,w", [(8, 16), (9, 17), (37, 53)])
def test_tail_backward_against_fp64(h, w, cout, n, padded):
    """df, dw, db against CPU fp64 autograd of the definition (8 x 16: one tile; 9 x 17: every tile edge; 37 x 53: 5 x 4 tiles); the
    forward under autograd has the bits of the no-grad call."""
    from isosurfacesuperresolution_amd import ops
    f, wt, b, dout = _tail_case(n, h, w, cout, padded, 1000 * h + 10 * w + cout)
    out, hip = _tail_grads(f, wt, b, dout, True)
    with torch.no_grad():
        assert torch.equal(out, ops.pixel_shuffle4_conv(f, wt, b))
    _, composite = _tail_grads(f, wt, b, dout, False)
    _, ref = _tail_grads(f.double().cpu(), wt.double().cpu(), b.double().cpu(), dout.double().cpu(), True)
    torch.cuda.synchronize()
    assert all(g.shape == r.shape and g.dtype == torch.float32 for g, r in zip(hip, ref))
    _judge("tail %dx%dx%d -> %d %s" % (n, h, w, cout, "padded" if padded else "packed"), TAIL_NAMES, hip, composite, ref)
    if padded:
        assert (f._whole == 1e30).sum().item() == f._whole.numel() - f.numel()


@pytest.mark.parametrize("h,w", [(8, 16), (9, 17)])
def test_tail_data_gradient_of_a_one_hot_is_the_weights(h, w):
    """dout one-hot at (co, Y, X): df's non-zeros are bitwise the 36 weights w[co][ci][ky][kx], at channel 16 ci + 4 i + j of pixel
    (y, x) with (4 y + i, 4 x + j) = (Y + ky - 1, X + kx - 1) -- fewer at an image border.  Corners, tile borders and the interior."""
    gen = torch.Generator().manual_seed(23)
    f = torch.randn(1, 64, h, w, generator=gen).cuda()
    wt = torch.randn(5, 4, 3, 3, generator=gen).cuda()
    b = torch.zeros(5, device="cuda")
    H, W, wt_host = 4 * h, 4 * w, wt.cpu()
    places = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (31, 63), (32, 64), (H // 2, 3), (5, W // 2)]
    for k, (Y, X) in enumerate(p for p in places if p[0] < H and p[1] < W):
        co = k % 5
        dout = torch.zeros(1, 5, H, W, device="cuda")
        dout[0, co, Y, X] = 1.0
        _, (df, _, _) = _tail_grads(f, wt, b, dout, True)
        want = torch.zeros(1, 64, h, w)
        for ci in range(4):
            for ky in range(3):
                for kx in range(3):
                    py, px = Y + ky - 1, X + kx - 1
                    if 0 <= py < H and 0 <= px < W:
                        want[0, 16 * ci + 4 * (py % 4) + px % 4, py // 4, px // 4] = wt_host[co, ci, ky, kx]
        assert torch.equal(df.cpu(), want), (Y, X, co)


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("n,h,w,cout", [(1, 8, 16, 3), (2, 9, 17, 8), (2, 37, 53, 5)])
def test_tail_weight_gradient_of_integers_is_exact(n, h, w, cout, padded):
    """Integer f in [-8, 8] and dout in [-3, 3]: every partial sum of dw and db stays below 2 x 24 x 148 x 212 < 2^24, so both equal
    fp64 exactly (and so does df: 9 Cout terms of at most 9)."""
    f, wt, b, dout = _tail_case(n, h, w, cout, padded, 41, integers=True)
    _, hip = _tail_grads(f, wt, b, dout, True)
    _, ref = _tail_grads(f.double().cpu(), wt.double().cpu(), b.double().cpu(), dout.double().cpu(), True)
    for name, g, r in zip(TAIL_NAMES, hip, ref):
        assert torch.equal(g.double().cpu(), r), name


# ------------------------------------------------------------------------------------------------------------------- determinism

def test_two_backward_runs_give_the_same_bits():
    gen = torch.Generator().manual_seed(77)
    x, t, dy = (_laid_out(torch.randn(2, 64, 67, 129, generator=gen), "padded") for _ in range(3))
    operands = (x, t) + _perceptron(gen, scale=3.0)
    first, second = _attention_grads(operands, dy, True)[1], _attention_grads(operands, dy, True)[1]
    for name, a, b in zip(ATT_NAMES, first, second):
        assert torch.equal(a, b), name
    f, wt, b, dout = _tail_case(2, 37, 53, 3, False, 78)
    first, second = _tail_grads(f, wt, b, dout, True)[1], _tail_grads(f, wt, b, dout, True)[1]
    for name, a, b in zip(TAIL_NAMES, first, second):
        assert torch.equal(a, b), name


def test_nothing_is_launched_for_gradients_nobody_needs():
    """``needs_input_grad``: only x needs a gradient -> no launch at all; only the perceptron -> the sums and the parameter launch; only t
    -> the sums and the streaming launch; the tail likewise."""
    from isosurfacesuperresolution_amd import ops
    gen = torch.Generator().manual_seed(5)
    x, t, dy = (torch.randn(2, 64, 9, 11, generator=gen).cuda() for _ in range(3))
    params = _perceptron(gen)

    def launched(needs, fn, operands, g):
        leaves = [v.detach().requires_grad_(k) for v, k in zip(operands, needs)]
        y = fn(*leaves)
        ops.profile_enable(True)
        try:
            y.backward(g)
            torch.cuda.synchronize()
            return [name for name, _, _ in ops.profile_records()]
        finally:
            ops.profile_enable(False)
    att = ops.channel_attention_residual
    assert launched((True, False, False, False, False, False), att, (x, t) + params, dy) == []
    assert launched((False, False, True, True, True, True), att, (x, t) + params, dy) == ["gate_grad_sum_kernel", "gate_param_grad_kernel"]
    assert launched((True, True, False, False, False, False), att, (x, t) + params, dy) == ["gate_grad_sum_kernel", "gate_backward_kernel"]
    f, wt, b, dout = _tail_case(1, 9, 17, 3, False, 6)
    tail = ops.pixel_shuffle4_conv
    assert launched((True, False, False), tail, (f, wt, b), dout) == ["shuffle_tail_dgrad_kernel"]
    assert launched((False, True, True), tail, (f, wt, b), dout) == ["shuffle_tail_wgrad_kernel", "shuffle_tail_wgrad_sum_kernel"]


# ----------------------------------------------------------------------------------------------------------------------- routing

def test_an_rcan_under_autograd_runs_on_the_kernels_of_the_package(monkeypatch):
    """1 x 2 blocks, forward and backward under the profiler with every PyTorch-route warning an error: the forward kernels once per
    block / once, every block's backward three launches, the tail's three; each node's forward output has the bits of the no-grad call
    on the same operands.  (The network's convolutions take the training kernels under autograd and the inference kernels without, so
    the comparison is made per node, where this change decides the bits.)"""
    from isosurfacesuperresolution_amd import ops, train
    net = small_rcan(1, 2).train().cuda()
    g = torch.Generator().manual_seed(4)
    x, target = torch.rand(2, 56, 8, 12, generator=g).cuda(), torch.rand(2, 3, 32, 48, generator=g).cuda()
    seen = []
    for name in ("channel_attention_residual", "pixel_shuffle4_conv"):
        def recorded(*a, _fn=getattr(ops, name), **kw):
            out = _fn(*a, **kw)
            seen.append((_fn, [v.detach() if torch.is_tensor(v) else v for v in a], kw, out))
            return out
        monkeypatch.setattr(ops, name, recorded)
    ops.profile_enable(True)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            pred, residual = net(x)
            loss = ((pred - target) ** 2).mean() + 0.1 * (residual ** 2).mean()
            train.backward(loss)
        torch.cuda.synchronize()
        names = [n for n, _, _ in ops.profile_records()]
    finally:
        ops.profile_enable(False)
    counts = {k: names.count(k) for k in ("channel_pool_kernel", "gate_scale_add_kernel", "shuffle_tail_kernel") + BACKWARD_KERNELS}
    assert counts == {"channel_pool_kernel": 2, "gate_scale_add_kernel": 2, "shuffle_tail_kernel": 1, "gate_grad_sum_kernel": 2,
                      "gate_backward_kernel": 2, "gate_param_grad_kernel": 2, "shuffle_tail_dgrad_kernel": 1,
                      "shuffle_tail_wgrad_kernel": 1, "shuffle_tail_wgrad_sum_kernel": 1}, counts
    assert len(seen) == 3
    with torch.no_grad():
        for fn, a, kw, out in seen:
            assert out.requires_grad and torch.equal(out, fn(*a, **kw))
    ops.range_reset()                                                 # (the no-grad calls armed the blocks' range words)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())


# --------------------------------------------------------------------------------------------------------------------- the clip

B, T, LOW, HIGH = 2, 3, 8, 32


def _clip(seed):
    g = torch.Generator().manual_seed(seed)
    inp = torch.rand(B, T, 8, LOW, LOW, generator=g)
    flow = (torch.rand(B, T, 2, LOW, LOW, generator=g) - 0.5) * 0.05
    tgt = torch.rand(B, T, 3, HIGH, HIGH, generator=g)
    return inp, flow, tgt


def _criterion(target, prediction, input_low, previous_warped):
    """L1 + 0.1 MSE against the warped previous frame."""
    return (prediction - target).abs().mean() + 0.1 * ((prediction - previous_warped) ** 2).mean(), {}


def test_colour_clip_gradients_on_the_hip_path_match_fp64_on_the_cpu():
    """A 1 x 2-block RCAN 56 -> 3, B = 2, T = 3, 8 x 8 -> 32 x 32 through ``train.colour_clip_loss``: loss and every parameter's gradient
    against the same clip on the CPU in fp64 at the bounds of tests/test_tecogan_train_gpu.py -- per-parameter relative norm max <= 1e-2,
    median <= 1e-3, loss <= 1e-5 relative."""
    from isosurfacesuperresolution_amd import train
    batch = _clip(3)
    net = small_rcan(1, 2).train()
    ref_net = copy.deepcopy(net).double()
    ref_loss, ref_sum = train.colour_clip_loss(ref_net, _criterion, *(t.double() for t in batch))
    ref_loss.backward()
    net = net.cuda()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        loss, loss_sum = train.colour_clip_loss(net, _criterion, *(t.cuda() for t in batch))
        train.backward(loss)
    assert abs(loss_sum.item() - ref_sum.item()) <= 1e-5 * max(1.0, abs(ref_sum.item()))
    errs = {}
    for (name, p), r in zip(net.named_parameters(), ref_net.parameters()):
        assert p.grad is not None and p.grad.shape == p.shape and r.grad.norm().item() > 0, name
        errs[name] = ((p.grad.cpu().double() - r.grad).norm() / r.grad.norm()).item()
    ranked = sorted(errs.items(), key=lambda kv: kv[1])
    print("RCAN clip gradients vs fp64: max %.3g (%s), median %.3g" % (ranked[-1][1], ranked[-1][0], ranked[len(ranked) // 2][1]))
    assert ranked[-1][1] <= 1e-2, ranked[-4:]
    assert ranked[len(ranked) // 2][1] <= 1e-3, ranked[-8:]


def test_graphed_colour_train_step_reproduces_the_eager_step_on_every_replay():
    """``GraphedTrainStep(..., clip_loss=train.colour_clip_loss)``: replay k leaves the gradients and the loss of eager step k at the
    bounds of the TecoGAN graph test (relative norm <= 1e-3, loss <= 1e-5 relative)."""
    from isosurfacesuperresolution_amd import train
    batch = tuple(t.cuda() for t in _clip(5))
    eager_net, graph_net = small_rcan(1, 2).train().cuda(), small_rcan(1, 2).train().cuda()
    eager_opt, _ = train.make_optimizer(eager_net, lr=1e-4, capturable=True, flat=True)
    graph_opt, _ = train.make_optimizer(graph_net, lr=1e-4, capturable=True, flat=True)
    step = train.GraphedTrainStep(graph_net, _criterion, graph_opt, batch, warmup=3, clip_loss=train.colour_clip_loss)
    for k in range(3):
        eager_opt.zero_grad()
        loss, loss_sum = train.colour_clip_loss(eager_net, _criterion, *batch)
        train.backward(loss)
        eager_loss = loss_sum.item() / T
        grads = [p.grad.detach().clone() for p in eager_net.parameters()]
        eager_opt.step()
        graph_loss = float(step(batch))
        torch.cuda.synchronize()
        assert abs(graph_loss - eager_loss) <= 1e-5 * max(1.0, abs(eager_loss)), (k, graph_loss, eager_loss)
        for (name, p), r in zip(graph_net.named_parameters(), grads):
            assert ((p.grad - r).norm() / r.norm()).item() <= 1e-3, (k, name)


def test_twenty_steps_on_one_colour_clip_lower_the_loss():
    from isosurfacesuperresolution_amd import train
    batch = tuple(t.cuda() for t in _clip(7))
    net = small_rcan(1, 2).train().cuda()
    optim, _ = train.make_optimizer(net, lr=1e-4)
    history = [train.train_step(net, _criterion, optim, batch, clip_loss=train.colour_clip_loss) for _ in range(20)]
    assert all(torch.isfinite(p).all() for p in net.parameters())
    assert history[-1] < history[0], history
