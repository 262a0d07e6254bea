"""GPU: the three kernels of csrc/sr_attention.hip behind ``ops.channel_pool``, ``ops.channel_attention_residual`` and
``ops.pixel_shuffle4_conv`` -- each against its fp64 definition with a bound derived from the documented order of its arithmetic, and
bitwise where the definition fixes the bits."""
import warnings

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                                                     # unit roundoff of fp32
SHAPES = [(2, 1, 1), (2, 3, 5), (2, 8, 12), (2, 17, 33), (2, 67, 129)]      # (N, H, W); 67 x 129: more than one slab per plane


def _tensor(gen, n, h, w, padded, integers=False):
    """fp32 [n, 64, h, w] on the device: packed, or with padded channel planes (plane stride a multiple of four floats, so that the
    16-byte path with its per-element rest is taken) whose pad holds 1e30 -- a kernel that reads the pad cannot pass."""
    v = torch.randint(-8, 9, (n, 64, h, w), generator=gen).float() if integers else torch.randn(n, 64, h, w, generator=gen)
    if not padded:
        return v.cuda()
    plane = h * w + (4 - h * w % 4) % 4 + 4
    buf = torch.full((n * 64 * plane,), 1e30, dtype=torch.float32, device="cuda")
    t = buf.as_strided((n, 64, h, w), (64 * plane, plane, w, 1))
    t.copy_(v)
    t._whole = buf
    return t


def _perceptron(gen, scale=1.0):
    wd = (torch.randn(4, 64, generator=gen) * scale / 8).cuda()
    bd = (torch.randn(4, generator=gen) * 0.1).cuda()
    wu = (torch.randn(64, 4, generator=gen) * scale / 2).cuda()
    bu = (torch.randn(64, generator=gen) * 0.1).cuda()
    return wd, bd, wu, bu


# ---------------------------------------------------------------------------------------------------------------------------- pool

@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_channel_pool_against_the_fp64_mean(n, h, w, padded):
    """fp64 accumulation and ONE rounding to fp32: |mean - mean64| <= 2^-23 mean|t| (the rounding alone is 2^-24 |mean|); two runs give
    the same bits."""
    from isosurfacesuperresolution_amd import ops
    t = _tensor(torch.Generator().manual_seed(h * w), n, h, w, padded)
    assert ops.channel_pool_supported(t)
    z = ops.channel_pool(t)
    again = ops.channel_pool(t)
    torch.cuda.synchronize()
    assert z.shape == (n, 64) and z.dtype == torch.float32
    assert torch.equal(z, again)
    want = t.double().mean(dim=(2, 3))
    err = (z.double() - want).abs()
    bound = 2.0 ** -23 * t.double().abs().mean(dim=(2, 3))
    print("pool %dx%dx%d %s: worst error / bound %.3g" % (n, h, w, "padded" if padded else "packed", (err / bound).max().item()))
    assert (err <= bound).all()
    slabs = ops._sr().isrChannelPoolSlabs(n, h, w)
    assert (slabs > 1) == (h * w > 4096)
    if padded:
        assert (t._whole == 1e30).sum().item() == t._whole.numel() - t.numel()          # nothing wrote the pad


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_channel_pool_of_small_integers_is_exact(n, h, w, padded):
    from isosurfacesuperresolution_amd import ops
    t = _tensor(torch.Generator().manual_seed(7), n, h, w, padded, integers=True)
    z = ops.channel_pool(t)
    assert torch.equal(z, (t.double().sum(dim=(2, 3)) / (h * w)).float())


# ---------------------------------------------------------------------------------------------------------------- gate, scale and add

def _gate_bound(z, wd, bd, wu, bu, slope):
    """-> (s64, bound): the fp64 gate from the fp32 mean ``z`` and the error bound of the kernel's documented order.  A chain of k
    fmaf's starting from the bias is within k 2^-24 sum|terms| of the exact sum (terms: the bias and the k products); the leaky
    multiply adds one rounding; the errors of the four hidden values reach u through |Wu|; the sigmoid's slope is at most 1/4; expf and
    the division are allowed 4 ulp (2^-23 s each)."""
    z, wd, bd, wu, bu = (v.double().cpu() for v in (z, wd, bd, wu, bu))
    a = z @ wd.t() + bd                                              # [N, 4]
    e_a = 64 * U * (z.abs() @ wd.abs().t() + bd.abs())
    g = torch.where(a > 0, a, a * slope)
    e_g = e_a + U * g.abs()
    u = g @ wu.t() + bu                                              # [N, 64]
    e_u = e_g @ wu.abs().t() + 4 * U * (g.abs() @ wu.abs().t() + bu.abs())
    s = torch.sigmoid(u)
    return s, 0.25 * e_u + 4 * 2.0 ** -23 * s


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_gate_and_scale_add(n, h, w, padded):
    """The gate against its fp64 definition evaluated at the kernel's own mean, bound per case from the operands; y bitwise
    ``x + t * s[:, :, None, None]`` with the kernel's exported s."""
    from isosurfacesuperresolution_amd import ops
    gen = torch.Generator().manual_seed(100 + h * w)
    x, t = _tensor(gen, n, h, w, padded), _tensor(gen, n, h, w, padded)
    t.add_(torch.randn(n, 64, 1, 1, generator=gen).cuda())          # per-channel means of order one: gates all over (0, 1)
    wd, bd, wu, bu = _perceptron(gen, scale=3.0)
    assert ops.channel_attention_supported(x, t, wd, wu)
    y, s = ops.channel_attention_residual(x, t, wd, bd, wu, bu, slope=0.01, return_gate=True)
    y_only = ops.channel_attention_residual(x, t, wd, bd, wu, bu, slope=0.01)
    z = ops.channel_pool(t)
    torch.cuda.synchronize()
    s64, bound = _gate_bound(z, wd, bd, wu, bu, 0.01)
    err = (s.double().cpu() - s64).abs()
    print("gate %dx%dx%d: worst error %.3g, worst error / bound %.3g, gates outside [0.25, 0.75]: %.0f %%"
          % (n, h, w, err.max().item(), (err / bound).max().item(), 100 * ((s < 0.25) | (s > 0.75)).float().mean().item()))
    assert (err <= bound).all()
    assert ((s < 0.25) | (s > 0.75)).float().mean().item() > 0.2          # a kernel that ignores the attention would be seen
    assert torch.equal(y, x + t * s[:, :, None, None])
    assert torch.equal(y, y_only)
    if padded:
        assert (x._whole == 1e30).sum().item() == x._whole.numel() - x.numel()


@pytest.mark.parametrize("h,w", [(3, 5), (8, 12), (67, 129)])
def test_scale_add_of_a_one_hot_lands_on_its_element(h, w):
    """t one-hot in each corner and in the last element of a row (x = 0): y is s[c] there and zero everywhere else."""
    from isosurfacesuperresolution_amd import ops
    gen = torch.Generator().manual_seed(5)
    wd, bd, wu, bu = _perceptron(gen)
    x = torch.zeros(1, 64, h, w, device="cuda")
    for c, (py, px) in zip((0, 13, 37, 63, 21), ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w - 1))):
        t = torch.zeros(1, 64, h, w, device="cuda")
        t[0, c, py, px] = 1.0
        y, s = ops.channel_attention_residual(x, t, wd, bd, wu, bu, return_gate=True)
        want = torch.zeros_like(y)
        want[0, c, py, px] = s[0, c]
        assert s[0, c].item() > 0 and torch.equal(y, want), (c, py, px)


def test_unsupported_operands_take_the_torch_composite():
    """Anything the kernels refuse (here 32 channels) runs the definition on the device."""
    from isosurfacesuperresolution_amd import ops
    gen = torch.Generator().manual_seed(9)
    x, t = torch.randn(1, 32, 6, 7, generator=gen).cuda(), torch.randn(1, 32, 6, 7, generator=gen).cuda()
    wd, bd, wu, bu = (torch.randn(s, generator=gen).cuda() for s in ((2, 32), (2,), (32, 2), (32,)))
    assert not ops.channel_attention_supported(x, t, wd, wu) and not ops.channel_pool_supported(t)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)             # (said once per process: "PyTorch operators run instead")
        y = ops.channel_attention_residual(x, t, wd, bd, wu, bu)
    s = torch.sigmoid(F.linear(F.leaky_relu(F.linear(t.mean(dim=(2, 3)), wd, bd), 0.01), wu, bu))
    assert (y - (x + t * s[:, :, None, None])).abs().max().item() <= 1e-6
    assert y._isr_range_key == ops.HOT


def test_range_word_of_the_gate_launch_routes_the_next_convolution():
    """The gate launch reports the largest |y| to the armed word (here: the word of a convolution weight, as models/rcan.py arms its
    block's second convolution again).  x of 4e4 makes the producer hot after ``refresh_range_flags``; the next ``conv3x3`` then takes
    the exact route.  With a small x nothing is hot and the consumer stays on the split kernel."""
    from isosurfacesuperresolution_amd import ops
    ops.range_reset()
    gen = torch.Generator().manual_seed(11)
    t = torch.randn(1, 64, 24, 40, generator=gen).cuda()
    wd, bd, wu, bu = _perceptron(gen)
    w_block = ((torch.rand(64, 64, 3, 3, generator=gen) - 0.5) * 0.05).cuda()        # stands for block.pre[2].weight: the key
    w_next = ((torch.rand(64, 64, 3, 3, generator=gen) - 0.5) * 0.05).cuda()
    dev = torch.device("cuda", torch.cuda.current_device())
    with torch.no_grad():
        small = torch.randn(1, 64, 24, 40, generator=gen).cuda()
        y = ops.channel_attention_residual(small, t, wd, bd, wu, bu, range_key=id(w_block))
        assert y._isr_range_key == id(w_block)
        assert not ops.refresh_range_flags(dev) and not ops.any_hot(dev)
        st = ops._range_state(dev)
        word = st["buf"][st["slots"][id(w_block)]:st["slots"][id(w_block)] + 1].view(torch.float32)
        assert word.item() == y.abs().max().item()                   # the word IS the largest |y| stored
        assert ops.conv3x3(y, w_next)._isr_range_key == id(w_next)   # split route
        x = small + 4.0e4
        y = ops.channel_attention_residual(x, t, wd, bd, wu, bu, range_key=id(w_block))
        new = ops.refresh_range_flags(dev)
        assert id(w_block) in new and ops.any_hot(dev) and ops.range_is_hot(y._isr_range_key, dev)
        assert word.item() == y.abs().max().item() >= 3.0e4
        out = ops.conv3x3(y, w_next)
        assert out._isr_range_key == ops.HOT                         # the exact fp32 kernel, and whatever consumes it stays exact
        # ... which propagates through the next block's gate launch
        y2 = ops.channel_attention_residual(out, t, wd, bd, wu, bu, range_key=id(w_next))
        assert y2._isr_range_key == ops.HOT
    ref = F.conv2d(y.double().cpu(), w_next.double().cpu(), padding=1)
    assert (out.double().cpu() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    ops.range_reset()
    assert not ops.any_hot(dev)


# --------------------------------------------------------------------------------------------------------------------- shuffle tail

TAIL_SHAPES = [(1, 1, 1, 3), (1, 2, 3, 3), (1, 5, 7, 3), (1, 8, 12, 3), (2, 19, 37, 3), (1, 17, 36, 3), (1, 5, 7, 6), (1, 9, 20, 8), (1, 3, 4, 1)]


def _tail_reference(f, w, b):
    """fp64 definition and the bound of the fmaf chain: 37 roundings (36 products + bias) -> 37 2^-24 sum|terms| per pixel."""
    p = F.pixel_shuffle(f.double().cpu(), 4)
    ref = F.conv2d(p, w.double().cpu(), b.double().cpu(), padding=1)
    terms = F.conv2d(p.abs(), w.double().cpu().abs(), b.double().cpu().abs(), padding=1)
    return ref, 37 * U * terms


@pytest.mark.parametrize("n,h,w,cout", TAIL_SHAPES)
def test_shuffle_tail_against_fp64(n, h, w, cout):
    """(19 x 37 and 17 x 36: three tiles of 8 x 16 in each direction, the second one on the 16-byte staging path.)"""
    from isosurfacesuperresolution_amd import ops
    gen = torch.Generator().manual_seed(h * 100 + w)
    f = torch.randn(n, 64, h, w, generator=gen).cuda()
    wt = (torch.randn(cout, 4, 3, 3, generator=gen) * 0.3).cuda()
    b = (torch.randn(cout, generator=gen) * 0.5 + 0.5).cuda()
    assert ops.pixel_shuffle4_conv_supported(f, wt)
    out = ops.pixel_shuffle4_conv(f, wt, b)
    clamped = ops.pixel_shuffle4_conv(f, wt, b, clamp=True)
    nobias = ops.pixel_shuffle4_conv(f, wt, None)
    torch.cuda.synchronize()
    assert out.shape == (n, cout, 4 * h, 4 * w) and out.is_contiguous()
    ref, bound = _tail_reference(f, wt, b)
    err = (out.double().cpu() - ref).abs()
    print("tail %dx%dx%d -> %d: worst error %.3g, worst error / bound %.3g" % (n, h, w, cout, err.max().item(), (err / bound).max().item()))
    assert (err <= bound).all()
    assert torch.equal(clamped, out.clamp(0, 1))
    if h * w >= 35:
        assert (out < 0).any() and (out > 1).any()                    # (the clamp had something to do)
    ref0, bound0 = _tail_reference(f, wt, torch.zeros_like(b))
    assert ((nobias.double().cpu() - ref0).abs() <= bound0).all()


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("n,h,w,cout", [(1, 5, 7, 3), (2, 19, 37, 3), (1, 17, 36, 3), (1, 9, 20, 8)])
def test_shuffle_tail_of_integers_is_exact(n, h, w, cout, padded):
    from isosurfacesuperresolution_amd import ops
    gen = torch.Generator().manual_seed(3)
    f = _tensor(gen, n, h, w, padded, integers=True)
    wt = torch.randint(-3, 4, (cout, 4, 3, 3), generator=gen).float().cuda()
    b = torch.randint(-5, 6, (cout,), generator=gen).float().cuda()
    out = ops.pixel_shuffle4_conv(f, wt, b)
    ref = F.conv2d(F.pixel_shuffle(f.double().cpu(), 4), wt.double().cpu(), b.double().cpu(), padding=1)
    assert torch.equal(out.double().cpu(), ref)


@pytest.mark.parametrize("h,w", [(5, 7), (19, 37)])
def test_shuffle_tail_one_hot_lands_on_one_pixel(h, w):
    """f one-hot in each of the 16 phases of every corner pixel, a one-hot weight (one tap, output channel 1): channel 16 c + 4 i + j of
    low-resolution pixel (y, x) is channel c at (4 y + i, 4 x + j), and tap (ky, kx) moves it to (4 y + i - ky + 1, 4 x + j - kx + 1)."""
    from isosurfacesuperresolution_amd import ops
    zero = torch.zeros(3, device="cuda")
    for corner, (y, x) in enumerate(((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1))):
        for phase in range(16):
            i, j, c = phase // 4, phase % 4, (corner + phase) % 4
            ky, kx = (phase + corner) % 3, (phase // 3) % 3
            f = torch.zeros(1, 64, h, w, device="cuda")
            f[0, 16 * c + 4 * i + j, y, x] = 2.0
            wt = torch.zeros(3, 4, 3, 3, device="cuda")
            wt[1, c, ky, kx] = 1.5
            out = ops.pixel_shuffle4_conv(f, wt, zero)
            want = torch.zeros_like(out)
            ty, tx = 4 * y + i - ky + 1, 4 * x + j - kx + 1
            if 0 <= ty < 4 * h and 0 <= tx < 4 * w:
                want[0, 1, ty, tx] = 3.0
            assert torch.equal(out, want), (y, x, phase, ky, kx, out.nonzero().tolist())


def test_shuffle_tail_refuses_what_it_cannot_take():
    from isosurfacesuperresolution_amd import ops
    f = torch.randn(1, 64, 4, 4).cuda()
    assert not ops.pixel_shuffle4_conv_supported(f, torch.randn(9, 4, 3, 3).cuda())
    assert not ops.pixel_shuffle4_conv_supported(f[:, :32], torch.randn(3, 2, 3, 3).cuda())
    assert not ops.pixel_shuffle4_conv_supported(f.double(), torch.randn(3, 4, 3, 3).cuda())
    wt, b = torch.randn(3, 4, 3, 3, dtype=torch.float64).cuda(), torch.randn(3, dtype=torch.float64).cuda()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        out = ops.pixel_shuffle4_conv(f.double(), wt, b)               # the torch composite on the device
    assert (out - F.conv2d(F.pixel_shuffle(f.double(), 4), wt, b, padding=1)).abs().max().item() <= 1e-12
