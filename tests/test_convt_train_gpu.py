"""GPU: the backward of the stride-2 transposed convolution (TecoGAN's learned x2 upsampling) on the HIP training kernels --
``isrConvTransposePhaseGradient`` (csrc/sr_train.hip), ``convt3x3s2_dgrad_split_kernel`` (csrc/sr_conv_transpose.hip), the weight
gradient through the convolution's segment kernels, and ``ops.conv_transpose3x3_s2`` under autograd -- against PyTorch in fp64 on
the CPU (the reference trains through ``nn.ConvTranspose2d``).

Shapes are (N, h, w) of the low-resolution input.  The kernels' tile is 4 x 32 low-resolution pixels, the data gradient's halo row
and column lie above and to the left: a single pixel; odd sizes; exactly one tile; one past it both ways (the halo comes from a
neighbour tile, the last tiles are ragged); several tiles both ways."""
import ctypes
import functools
import warnings

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 3, 5), (1, 4, 32), (1, 5, 33), (1, 9, 70)]
DGRAD = "convt3x3s2_dgrad_split_kernel"
SLOPE = 0.01


def _convt64(x, w, b=None):
    return F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1)


@functools.lru_cache(maxsize=None)
def _case(n, h, w):
    """Normal input and output gradient, weights at the He scale sqrt(2 / (9 * 64)), a bias; and, in fp64 on the CPU (computed once
    per shape): the pre-activation z, and for a LeakyReLU layer y, gx, gW, gb.  The output gradient is ZERO where |z| < 1e-3: the
    activation's derivative jumps at 0, and a kernel result within rounding of the fp64 one may sit on the other side."""
    g = torch.Generator().manual_seed(10000 * n + 100 * h + w)
    x = torch.randn(n, 64, h, w, generator=g)
    wt = torch.randn(64, 64, 3, 3, generator=g) * (2.0 / (9 * 64)) ** 0.5
    b = torch.randn(64, generator=g) * 0.05
    gy = torch.randn(n, 64, 2 * h, 2 * w, generator=g)
    ref = [t.double().requires_grad_(True) for t in (x, wt, b)]
    z = _convt64(*ref)
    gy = torch.where(z.detach().abs() < 1e-3, torch.zeros_like(gy), gy)
    y = F.leaky_relu(z, SLOPE)
    gx, gw, gb = torch.autograd.grad(y, ref, gy.double())
    return {"x": x, "w": wt, "b": b, "gy": gy, "z": z.detach(), "y": y.detach(), "gx": gx, "gw": gw, "gb": gb}


def _gz64(c):
    return torch.where(c["z"] > 0, c["gy"].double(), c["gy"].double() * SLOPE)


@pytest.mark.parametrize("n,h,w", SHAPES)
@pytest.mark.parametrize("act", ["none", "leaky"])
def test_phase_gradient_kernel_equals_act_backward_then_pixel_unshuffle(n, h, w, act):
    from isosurfacesuperresolution_amd import ops
    c = _case(n, h, w)
    gy, y = c["gy"].cuda(), c["y"].float().cuda()
    y[0, 0, 0, 0] = 0.0                                                   # y == 0 is on the slope side
    gz = torch.empty_like(gy)
    rc = ops._sr().isrActBackward(ops._ptr(gy), ops._ptr(y), ops._ptr(gz), gy.numel(), ops.ACT_CODES[act], SLOPE, ops._stream())
    assert rc == 0
    got = ops.conv_transpose_phase_gradient(gy, None if act == 'none' else y, act, SLOPE)
    assert got.shape == (n, 256, h, w) and got.is_contiguous()
    assert torch.equal(got, F.pixel_unshuffle(gz, 2))
    if act == 'leaky':
        assert (y <= 0).any() and (y > 0).any()
    # a view that is only 4-byte aligned takes the dword path: the same bits
    if h * w > 1:
        flat = torch.empty(gy.numel() + 1, device="cuda")
        odd = flat[1:].view_as(gy).copy_(gy)
        assert odd.data_ptr() % 8 == 4
        assert torch.equal(ops.conv_transpose_phase_gradient(odd, None if act == 'none' else y, act, SLOPE), got)


def _data_grad(g, wd, words=None):
    """``ops._convt_data_grad`` under the profiler; with ``words`` (a zeroed int32 tensor) the launch is armed with the per-wave maxima."""
    from isosurfacesuperresolution_amd import ops
    used = 0
    ops.profile_enable(True)
    try:
        if words is not None:
            ops._sr().isrSetMaxSlots(ctypes.c_void_p(words.data_ptr()), words.numel())
        gx = ops._convt_data_grad(g, wd)
        if words is not None:
            used = ops._sr().isrTakeMaxSlotWords()
        torch.cuda.synchronize()
        names = [name for name, _, _ in ops.profile_records()]
    finally:
        ops.profile_enable(False)
    assert names == [DGRAD], names
    return gx, used


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_data_gradient_matches_fp64(n, h, w):
    """gx against the adjoint in fp64: <= 1e-4 max(1, max |ref|), the bound of test_residual_block_function_matches_fp64; the launch
    leaves the maximum of what it stored in the per-wave words; a second run gives the same bits."""
    from isosurfacesuperresolution_amd import ops
    c = _case(n, h, w)
    gz = _gz64(c)
    ref = F.conv2d(gz, c["w"].double(), stride=2, padding=1)              # the adjoint of conv_transpose2d: weight [ci, co] as [out, in]
    assert ref.shape == (n, 64, h, w)
    assert (ref - c["gx"]).abs().max().item() <= 1e-12 * max(1.0, c["gx"].abs().max().item())
    g = F.pixel_unshuffle(gz.float(), 2).contiguous().cuda()
    wd = c["w"].cuda()
    words = torch.zeros(8192, dtype=torch.int32, device="cuda")
    gx, used = _data_grad(g, wd, words)
    err = (gx.cpu().double() - ref).abs().max().item()
    print("convT dgrad %s: max error %.3g, max |ref| %.3g" % ((n, h, w), err, ref.abs().max().item()))
    assert err <= 1e-4 * max(1.0, ref.abs().max().item())
    tiles = n * ((h + 3) // 4) * ((w + 31) // 32)
    assert used == 4 * tiles
    assert words[used:].abs().max().item() == 0
    assert words[:used].max().item() == gx.abs().max().view(torch.int32).item()
    again, _ = _data_grad(g, wd)
    assert torch.equal(again, gx)


@pytest.mark.parametrize("h,w", [(1, 1), (4, 32), (5, 33)])
def test_data_gradient_of_small_integers_is_exact(h, w):
    """Small integers, every partial sum below 2^24: gx equals the fp64 result bit for bit.  A one-hot gz at each of the four image
    corners -- (0, 0), (0, 2w - 1), (2h - 1, 0), (2h - 1, 2w - 1): the four phases -- and a dense gradient: a wrong tap, flip, phase or
    halo side cannot hide in a tolerance."""
    g = torch.Generator().manual_seed(77 * h + w)
    wt = torch.randint(-4, 5, (64, 64, 3, 3), generator=g).float()
    wd = wt.cuda()
    cases = []
    for k, (yy, xx) in enumerate(((0, 0), (0, 2 * w - 1), (2 * h - 1, 0), (2 * h - 1, 2 * w - 1))):
        gz = torch.zeros(1, 64, 2 * h, 2 * w)
        gz[0, (17 * k + 5) % 64, yy, xx] = float(k + 2)
        cases.append(("corner (%d, %d)" % (yy, xx), gz))
    cases.append(("dense", torch.randint(-4, 5, (1, 64, 2 * h, 2 * w), generator=g).float()))      # |sum| <= 9 * 64 * 16 < 2^24
    for name, gz in cases:
        ref = F.conv2d(gz.double(), wt.double(), stride=2, padding=1)
        assert ref.abs().max().item() > 0, name
        gx, _ = _data_grad(F.pixel_unshuffle(gz, 2).contiguous().cuda(), wd)
        assert torch.equal(gx.cpu().double(), ref), name


@pytest.mark.parametrize("n,h,w", SHAPES)
@pytest.mark.parametrize("segments", [1, 3])
def test_weight_and_bias_gradient_match_fp64(n, h, w, segments):
    """(x, G) as a 64 -> 256 3x3 layer on the segment kernels, the live taps gathered: <= 1e-5 max |ref|, the bound of
    test_weight_gradient_over_segments_matches_fp64."""
    from isosurfacesuperresolution_amd import ops
    c = _case(n, h, w)
    g = torch.Generator().manual_seed(segments)
    xs = [c["x"]] + [torch.randn(n, 64, h, w, generator=g) for _ in range(segments - 1)]
    gzs = [_gz64(c).float()] + [torch.randn(n, 64, 2 * h, 2 * w, generator=g) for _ in range(segments - 1)]
    wref = torch.zeros(64, 64, 3, 3, dtype=torch.float64, requires_grad=True)
    bref = torch.zeros(64, dtype=torch.float64, requires_grad=True)
    for x, gz in zip(xs, gzs):
        (_convt64(x.double(), wref, bref) * gz.double()).sum().backward()
    weight = torch.zeros(64, 64, 3, 3, device="cuda")
    gw, gb = ops._convt_weight_grad([x.cuda() for x in xs], [F.pixel_unshuffle(gz, 2).contiguous().cuda() for gz in gzs], weight, True)
    assert gw.shape == (64, 64, 3, 3) and gb.shape == (64,)
    ew = (gw.cpu().double() - wref.grad).abs().max().item()
    eb = (gb.cpu().double() - bref.grad).abs().max().item()
    print("convT wgrad %s x %d: dW %.3g of %.3g, db %.3g of %.3g" % ((n, h, w), segments, ew, wref.grad.abs().max().item(), eb, bref.grad.abs().max().item()))
    assert ew <= 1e-5 * wref.grad.abs().max().item()
    assert eb <= 1e-5 * bref.grad.abs().max().item()


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_whole_op_matches_fp64(n, h, w):
    """y, gx, gW, gb of ``ops.conv_transpose3x3_s2`` + LeakyReLU under autograd against fp64 ``F.conv_transpose2d`` + ``leaky_relu``:
    y and gx (split-operand arithmetic) within 1e-4 max(1, max |ref|), gW and gb (exact fp32 sums) within 1e-5 max |ref|.  Without a
    gradient for x no data-gradient launch is made."""
    from isosurfacesuperresolution_amd import ops
    c = _case(n, h, w)
    dev = [c[k].cuda().requires_grad_(True) for k in ("x", "w", "b")]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        y = ops.conv_transpose3x3_s2(*dev, act='leaky', slope=SLOPE)
        y.backward(c["gy"].cuda())
    assert y.shape == (n, 64, 2 * h, 2 * w) and y.is_contiguous()
    assert (y.detach().cpu().double() - c["y"]).abs().max().item() <= 1e-4 * max(1.0, c["y"].abs().max().item())
    assert (dev[0].grad.cpu().double() - c["gx"]).abs().max().item() <= 1e-4 * max(1.0, c["gx"].abs().max().item())
    assert (dev[1].grad.cpu().double() - c["gw"]).abs().max().item() <= 1e-5 * c["gw"].abs().max().item()
    assert (dev[2].grad.cpu().double() - c["gb"]).abs().max().item() <= 1e-5 * c["gb"].abs().max().item()
    # x needs no gradient: the weight gradient alone
    xd = c["x"].cuda()
    wd, bd = (c[k].cuda().requires_grad_(True) for k in ("w", "b"))
    ops.profile_enable(True)
    try:
        ops.conv_transpose3x3_s2(xd, wd, bd, act='leaky', slope=SLOPE).backward(c["gy"].cuda())
        torch.cuda.synchronize()
        names = [name for name, _, _ in ops.profile_records()]
    finally:
        ops.profile_enable(False)
    assert "convt3x3s2_split_kernel" in names and DGRAD not in names, names
    assert torch.equal(wd.grad, dev[1].grad) and torch.equal(bd.grad, dev[2].grad)


def test_deferred_weight_gradients_equal_per_frame_accumulation_and_repeat_bit_for_bit():
    """Three frames through ONE layer: inside ``deferred_weight_gradients()`` the layer gets one weight-gradient pass over all frames
    and ``weight.grad`` / ``bias.grad`` arrive in the ConvTranspose2d layout -- the per-frame sums in another order (relative norm
    <= 1e-5); a second run gives the same bits everywhere (fixed summation order, no float atomics)."""
    from isosurfacesuperresolution_amd import ops
    c = _case(2, 3, 5)
    g = torch.Generator().manual_seed(4)
    frames = [c["x"].cuda()] + [torch.randn(2, 64, 3, 5, generator=g).cuda() for _ in range(2)]
    gys = [c["gy"].cuda()] + [torch.randn(2, 64, 6, 10, generator=g).cuda() for _ in range(2)]

    def run(deferred):
        wd, bd = (c[k].cuda().requires_grad_(True) for k in ("w", "b"))
        xs = [f.clone().requires_grad_(True) for f in frames]
        loss = sum((ops.conv_transpose3x3_s2(x, wd, bd, act='leaky', slope=SLOPE) * gy).sum() for x, gy in zip(xs, gys))
        if deferred:
            with ops.deferred_weight_gradients():
                loss.backward()
        else:
            loss.backward()
        return [wd.grad, bd.grad] + [x.grad for x in xs]

    per_frame, deferred, again = run(False), run(True), run(True)
    assert deferred[0].shape == (64, 64, 3, 3) and deferred[1].shape == (64,)
    for a, b in zip(per_frame[:2], deferred[:2]):
        assert ((a - b).norm() / a.norm()).item() <= 1e-5
    for a, b in zip(per_frame[2:], deferred[2:]):
        assert torch.equal(a, b)                                          # the data gradients do not depend on the context
    for a, b in zip(deferred, again):
        assert torch.equal(a, b)
    # a parameter that carries a hook keeps the per-frame path: its gradient passes through autograd inside the context
    wd, bd = (c[k].cuda().requires_grad_(True) for k in ("w", "b"))
    seen = []
    wd.register_hook(lambda grad: seen.append(grad.shape))
    with ops.deferred_weight_gradients():
        (ops.conv_transpose3x3_s2(frames[0], wd, bd, act='leaky', slope=SLOPE) * gys[0]).sum().backward()
    assert seen == [torch.Size([64, 64, 3, 3])] and wd.grad is not None and bd.grad is not None


def test_routes_under_autograd():
    """64 -> 64: no fallback warning, and the step's flop tally grows by exactly the TRUE data-gradient count under "split" (the weight
    gradient of these few pixels runs on the exact kernels, with the embedded count).  32 -> 32: PyTorch's route and its warning, as
    before, and gradients that match fp64."""
    from isosurfacesuperresolution_amd import ops
    n, h, w = 2, 3, 5
    c = _case(n, h, w)
    dev = [c[k].cuda().requires_grad_(True) for k in ("x", "w", "b")]
    saved = ops.FLOP_TALLY
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            ops._warned.discard("convt_autograd")
            y = ops.conv_transpose3x3_s2(*dev, act='leaky', slope=SLOPE)
            ops.FLOP_TALLY = {}
            y.backward(c["gy"].cuda())
            tally = dict(ops.FLOP_TALLY)
    finally:
        ops.FLOP_TALLY = saved
    assert tally.get("split", 0.0) == 2.0 * 9 * 64 * 64 * n * h * w, tally
    assert tally.get("exact", 0.0) == 2.0 * 9 * 64 * 256 * n * h * w, tally
    assert "convt_autograd" not in ops._warned

    g = torch.Generator().manual_seed(32)
    x = torch.randn(1, 32, 3, 5, generator=g)
    wt = torch.randn(32, 32, 3, 3, generator=g) * 0.08
    b = torch.randn(32, generator=g) * 0.05
    gy = torch.randn(1, 32, 6, 10, generator=g)
    small = [t.cuda().requires_grad_(True) for t in (x, wt, b)]
    with pytest.warns(RuntimeWarning, match="PyTorch's own kernels"):
        ys = ops.conv_transpose3x3_s2(*small, act='none')
    ys.backward(gy.cuda())
    ref = [t.double().requires_grad_(True) for t in (x, wt, b)]
    _convt64(*ref).backward(gy.double())
    for a, r in zip(small, ref):
        assert (a.grad.cpu().double() - r.grad).abs().max().item() <= 1e-4 * max(1.0, r.grad.abs().max().item())
