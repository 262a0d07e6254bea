"""The stride-2 3x3 convolution of the discriminators (``ops.conv3x3_s2``, csrc/sr_conv_stride2.hip): forward, data gradient and
weight gradient, one launch at a time against fp64 torch, then the autograd node, the deferred weight gradient, the two baseline
routes and the fall-back for shapes the kernels do not take.

Shapes (N, Cin, Cout, H, W): 2 x 2 and 4 x 4 outputs (a pixel tile spans several images), non-square images, pixel counts that are
no multiple of the 64- and 128-pixel tiles or of the weight gradient's 32-pixel chunks, every channel tile (16, 32, 64 wide), Cin !=
Cout and the widest channels.

Bars, none of them taken from the kernels under test (tests/test_train_routes_gpu.py, tests/test_convt_train_gpu.py):
    values and data gradients     max |y - ref| <= 1e-4  and  max |y - ref| / max |ref| <= 2e-6 max(1, K / 576), K = 9 x inputs of the launch
    weight and bias gradients     max |d - ref| <= 1e-5 max |ref|, with 1 and with 3 segments
The errors are printed for the first and last rows and columns (where the padding, or the missing tap of the data gradient, sits) and
for the whole tensor separately."""
import functools
import warnings

import pytest
import torch
import torch.nn.functional as F

from train_route_common import observed

pytestmark = pytest.mark.gpu

CASES = [(1, 32, 16, 4, 4), (3, 16, 16, 16, 16), (2, 32, 32, 12, 40), (2, 64, 64, 8, 8), (3, 256, 256, 8, 8), (2, 128, 128, 20, 72)]
IDS = ["%dx%d-%d-%dx%d" % (n, cin, cout, h, w) for n, cin, cout, h, w in CASES]
SLOPE = 0.01
KERNELS = {"fwd": "conv3x3s2_fwd_kernel", "dgrad": "conv3x3s2_dgrad_kernel", "wgrad": "conv3x3s2_wgrad_kernel"}


@functools.lru_cache(maxsize=None)
def _data(case):
    """Operands (fp32, CPU) of three segments and the fp64 references of one case; computed once, never written to."""
    n, cin, cout, h, w = case
    g = torch.Generator().manual_seed(1000 * cin + 10 * cout + h)
    u = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    t = {"w": u(cout, cin, 3, 3) / (3.0 * cin ** 0.5), "b": torch.rand(cout, generator=g) - 0.5,
         "xs": [u(n, cin, h, w) for _ in range(3)], "gs": [u(n, cout, h // 2, w // 2) for _ in range(3)]}
    x, gz, wd = t["xs"][0].double(), t["gs"][0].double(), t["w"].double()
    t["y"] = F.leaky_relu(F.conv2d(x, wd, t["b"].double(), stride=2, padding=1), SLOPE)
    t["y_plain"] = F.conv2d(x, wd, None, stride=2, padding=1)
    t["gx"] = F.conv_transpose2d(gz, wd, stride=2, padding=1, output_padding=1)
    dws = [torch.nn.grad.conv2d_weight(a.double(), wd.shape, b.double(), stride=2, padding=1) for a, b in zip(t["xs"], t["gs"])]
    dbs = [b.double().sum(dim=(0, 2, 3)) for b in t["gs"]]
    t["dw"] = {1: dws[0], 3: dws[0] + dws[1] + dws[2]}
    t["db"] = {1: dbs[0], 3: dbs[0] + dbs[1] + dbs[2]}
    return t


def _check_values(what, got, ref, inputs):
    got = got.double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    edge = torch.zeros_like(err, dtype=torch.bool)
    edge[..., 0, :] = edge[..., -1, :] = edge[..., :, 0] = edge[..., :, -1] = True
    scale = ref.abs().max().item()
    bar = 2e-6 * max(1.0, 9.0 * inputs / 576.0)
    for name, e in (("edges", err[edge].max().item()), ("whole", err.max().item())):
        print("%s %s: max error %.3e, normalised %.3e (bars 1e-4, %.1e)" % (what, name, e, e / scale, bar))
    assert err.max().item() <= 1e-4, what
    assert err.max().item() / scale <= bar, what


def _check_param_grad(what, got, ref):
    err = (got.double().cpu() - ref).abs().max().item()
    scale = ref.abs().max().item()
    print("%s: max error %.3e of %.3e (bar 1e-5 relative)" % (what, err, scale))
    assert err <= 1e-5 * scale, what


def _flops(case):
    n, cin, cout, h, w = case
    return 2.0 * 9 * cin * cout * n * (h // 2) * (w // 2)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_matches_fp64_and_repeats_bit_for_bit(case):
    from isosurfacesuperresolution_amd import ops
    t = _data(case)
    x, w, b = t["xs"][0].cuda(), t["w"].cuda(), t["b"].cuda()
    assert ops.conv_s2_supported(x, w)
    with torch.no_grad():
        y, families, names = observed(lambda: ops.conv3x3_s2(x, w, b, act='leaky', slope=SLOPE))
        # nine products per output pixel on the exact family, on the stride-2 kernel: the embedded form would tally four times that
        assert families == {"exact": _flops(case)} and names == [KERNELS["fwd"]], (families, names)
        _check_values("forward leaky", y, t["y"], case[1])
        _check_values("forward plain", ops.conv3x3_s2(x, w), t["y_plain"], case[1])
        assert torch.equal(y, ops.conv3x3_s2(x, w, b, act='leaky', slope=SLOPE))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_data_gradient_matches_fp64_and_repeats_bit_for_bit(case):
    from isosurfacesuperresolution_amd import ops
    n, cin, cout, h, w = case
    t = _data(case)
    gz, wt = t["gs"][0].cuda(), t["w"].cuda()
    gx, families, names = observed(lambda: ops._conv_s2_data_grad(gz, wt, h, w))
    assert families == {"exact": _flops(case)} and names == [KERNELS["dgrad"]], (families, names)
    _check_values("data gradient", gx, t["gx"], cout)
    assert torch.equal(gx, ops._conv_s2_data_grad(gz, wt, h, w))


@pytest.mark.parametrize("segments", [1, 3])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_weight_gradient_matches_fp64_and_repeats_bit_for_bit(case, segments):
    from isosurfacesuperresolution_amd import ops
    t = _data(case)
    xs, gs, wt = [a.cuda() for a in t["xs"][:segments]], [a.cuda() for a in t["gs"][:segments]], t["w"].cuda()
    (dw, db), families, names = observed(lambda: ops._conv_s2_weight_grad(xs, gs, wt, True))
    assert families == {"exact": segments * _flops(case)}, families
    assert names == [KERNELS["wgrad"], "conv3x3s2_wgrad_sum_kernel"], names
    _check_param_grad("weight gradient, %d segment(s)" % segments, dw, t["dw"][segments])
    _check_param_grad("bias gradient, %d segment(s)" % segments, db, t["db"][segments])
    dw2, db2 = ops._conv_s2_weight_grad(xs, gs, wt, True)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


def _autograd(case, frames, deferred=False):
    """Sum over ``frames`` of <conv3x3_s2(x_k), g_k> differentiated: (y_0, [gx_k], dw, db) on the device."""
    from isosurfacesuperresolution_amd import ops
    t = _data(case)
    w = t["w"].cuda().requires_grad_(True)
    b = t["b"].cuda().requires_grad_(True)
    xs = [a.cuda().requires_grad_(True) for a in t["xs"][:frames]]
    ctx = ops.deferred_weight_gradients() if deferred else warnings.catch_warnings()
    with ctx:
        ys = [ops.conv3x3_s2(x, w, b, act='leaky', slope=SLOPE) for x in xs]
        sum((y * g.cuda()).sum() for y, g in zip(ys, t["gs"])).backward()
    return ys[0].detach(), [x.grad for x in xs], w.grad, b.grad


@pytest.mark.parametrize("case", [CASES[2], CASES[4]], ids=[IDS[2], IDS[4]])
def test_autograd_gives_the_same_tensors_as_the_pieces(case):
    from isosurfacesuperresolution_amd import ops
    n, cin, cout, h, w = case
    t = _data(case)
    (y, gxs, dw, db), families, names = observed(lambda: _autograd(case, 1))
    assert set(families) == {"exact"} and families["exact"] == 3 * _flops(case), families
    assert [k for k in names if k.startswith("conv3x3")] == [KERNELS["fwd"], KERNELS["dgrad"], KERNELS["wgrad"], "conv3x3s2_wgrad_sum_kernel"], names
    wt, bt, x = t["w"].cuda(), t["b"].cuda(), t["xs"][0].cuda()
    with torch.no_grad():
        y_piece = ops.conv3x3_s2(x, wt, bt, act='leaky', slope=SLOPE)
    gz = torch.where(y_piece > 0, t["gs"][0].cuda(), t["gs"][0].cuda() * SLOPE)
    assert torch.equal(y, y_piece)
    assert torch.equal(gxs[0], ops._conv_s2_data_grad(gz, wt, h, w))
    dw_piece, db_piece = ops._conv_s2_weight_grad([x], [gz], wt, True)
    assert torch.equal(dw, dw_piece) and torch.equal(db, db_piece)
    # ... and against fp64 autograd of the whole node
    x64 = t["xs"][0].double().requires_grad_(True)
    w64, b64 = t["w"].double().requires_grad_(True), t["b"].double().requires_grad_(True)
    (F.leaky_relu(F.conv2d(x64, w64, b64, stride=2, padding=1), SLOPE) * t["gs"][0].double()).sum().backward()
    _check_values("autograd input gradient", gxs[0], x64.grad, cout)
    _check_param_grad("autograd weight gradient", dw, w64.grad)
    _check_param_grad("autograd bias gradient", db, b64.grad)


@pytest.mark.parametrize("case", [CASES[1], CASES[3]], ids=[IDS[1], IDS[3]])
def test_deferred_and_per_frame_weight_gradients_agree(case):
    _, gx_a, dw_a, db_a = _autograd(case, 3)
    (_, gx_b, dw_b, db_b), _, names = observed(lambda: _autograd(case, 3, deferred=True))
    assert names.count(KERNELS["wgrad"]) == 1 and names.count(KERNELS["fwd"]) == 3, names      # one pass over the three frames
    for a, b in zip(gx_a, gx_b):
        assert torch.equal(a, b)
    for a, b in ((dw_a, dw_b), (db_a, db_b)):
        assert ((a - b).norm() / a.norm()).item() <= 1e-5


@pytest.mark.parametrize("route", ["embedded", "torch"])
@pytest.mark.parametrize("case", [CASES[1], CASES[2], CASES[3]], ids=[IDS[1], IDS[2], IDS[3]])
def test_baseline_routes_meet_the_same_bars(case, route, monkeypatch):
    from isosurfacesuperresolution_amd import ops
    monkeypatch.setattr(ops, "CONV_S2_ROUTE", route)
    t = _data(case)
    (y, gxs, dw, db), _, names = observed(lambda: _autograd(case, 1))
    assert not any(k.startswith("conv3x3s2") for k in names), names
    x64 = t["xs"][0].double().requires_grad_(True)
    w64, b64 = t["w"].double().requires_grad_(True), t["b"].double().requires_grad_(True)
    (F.leaky_relu(F.conv2d(x64, w64, b64, stride=2, padding=1), SLOPE) * t["gs"][0].double()).sum().backward()
    _check_values(route + " forward", y, t["y"], case[1])
    _check_values(route + " input gradient", gxs[0], x64.grad, case[2])
    _check_param_grad(route + " weight gradient", dw, w64.grad)
    _check_param_grad(route + " bias gradient", db, b64.grad)


def test_an_odd_sized_input_warns_once_and_meets_the_bars(monkeypatch):
    from isosurfacesuperresolution_amd import ops
    monkeypatch.setattr(ops, "_warned", set(ops._warned) - {"conv_s2_shape"})           # as in a fresh process
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, 16, 9, 14, generator=g) * 2 - 1
    w = (torch.rand(32, 16, 3, 3, generator=g) * 2 - 1) / 12.0
    xd, wd = x.cuda(), w.cuda()
    assert not ops.conv_s2_supported(xd, wd)
    assert not ops.conv_s2_supported(torch.empty(1, 24, 8, 8, device="cuda"), torch.empty(16, 24, 3, 3, device="cuda"))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        y = ops.conv3x3_s2(xd, wd, act='leaky', slope=SLOPE)
        ops.conv3x3_s2(xd, wd, act='leaky', slope=SLOPE)
    assert len([c for c in caught if "conv3x3_s2" in str(c.message)]) == 1, [str(c.message) for c in caught]
    _check_values("odd size", y, F.leaky_relu(F.conv2d(x.double(), w.double(), stride=2, padding=1), SLOPE), 16)
