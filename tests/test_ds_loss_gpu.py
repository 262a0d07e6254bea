"""GPU: the downsample-consistency terms (``l2-ds`` / ``l1-ds``) of ``LossNetUnshaded`` on the fused path -- ``ops.loss_unshaded_ds``,
``isrLossDownsampleForward`` / ``isrLossDownsampleBackward`` of csrc/sr_train.hip -- against values recorded from the reference's own
modules (tests/golden/make_ds_fixtures.py) and against the module path in fp64 on the same inputs."""
import functools

import numpy as np
import pytest
import torch

import ds_common

pytestmark = pytest.mark.gpu

DS_ONLY = ds_common.DS_TERMS
FULL = ds_common.RECIPE + "," + ds_common.DS_TERMS
L2_ONLY = "l2-ds:mask:0.7,l2-ds:normal:1.3,l2-ds:depth:0.9,l2-ds:color:1.1"
UPSTREAM = 1.7


def _criterion(device, spec, size, padding, ao=0.5, inverse_ao=False):
    from isosurfacesuperresolution_amd import losses
    crit = losses.LossNetUnshaded(device, 5, 6, size, padding, ds_common.options(spec, ao=ao)).to(device)
    crit.shading.inverse_ao = inverse_ao
    return crit


@functools.lru_cache(maxsize=None)
def _inputs(n, h, w, seed):
    """gt, pred, input, prev (CPU fp32; shared, never modified).  The input's mask is drawn from [-1.5, 1.5): the gate clamps on both
    sides; the prediction's AO from [-0.2, 1.2): so does the shader's.  Zero normals in the prediction and in the input (the 1e-7 floor
    of the normalisation), and one cell in which the prediction's mask equals the input's."""
    rs = np.random.RandomState(seed)
    gt, pred, prev = (torch.from_numpy(rs.uniform(-1.0, 1.0, (n, 6, h, w)).astype(np.float32)) for _ in range(3))
    inp = torch.from_numpy(rs.uniform(-1.0, 1.0, (n, 5, h, w)).astype(np.float32))
    inp[:, 0] *= 1.5
    pred[:, 5] = pred[:, 5] * 0.7 + 0.5
    pred[:, 1:4, 1, 1] = 0.0
    inp[:, 1:4, 2, 2] = 0.0
    if h >= 8 and w >= 8:
        pred[:, 1:4, 4:8, 4:8] = 0.0
        inp[:, 1:4, 0:4, 4:8] = 0.0
    if h >= 12:
        pred[:, 0, 8:12, 4:8] = inp[:, 0, 8:12, 4:8]
    return gt, pred, inp, prev


def _odd_view(t):
    """``t`` as a contiguous view that starts 4 bytes into its storage."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _run(crit, tensors, device, dtype, with_prev, odd_views=False):
    gt, pred, inp, prev = (t.to(device=device, dtype=dtype) for t in tensors)
    if odd_views:
        gt, pred, inp, prev = (_odd_view(t) for t in (gt, pred, inp, prev))
    pred = pred.detach().requires_grad_(True)
    prev = prev.detach().requires_grad_(True) if with_prev else None
    total, values = crit(gt, pred, inp, None, prev)
    (total * UPSTREAM).backward()
    return total.item(), {k: float(v) for k, v in values.items()}, pred.grad, prev.grad if with_prev else None


def _l1_ds_differences(crit, pred, inp):
    """The differences that the enabled l1-ds terms take the absolute value of, with the module path's own operators."""
    from isosurfacesuperresolution_amd.losses import LossNetUnshaded
    from isosurfacesuperresolution_amd.utils import ScreenSpaceShading
    if "l1-ds" not in crit.loss_dict:
        return {}
    pred = LossNetUnshaded.pad(pred, crit.padding)
    norm, sample = ScreenSpaceShading.normalize, crit.loss_dict["l1-ds"].sample
    gate = torch.clamp(inp[:, 0:1] * 0.5 + 0.5, 0, 1)
    pairs = {"mask": lambda: (inp[:, 0:1], pred[:, 0:1]), "normal": lambda: (norm(inp[:, 1:4], dim=1) * gate, norm(pred[:, 1:4], dim=1) * gate),
             "depth": lambda: (inp[:, 4:5] * gate, pred[:, 4:5] * gate), "color": lambda: (crit.shading(inp), crit.shading(pred))}
    out = {}
    for target, pair in pairs.items():
        if ("l1-ds", target) in crit.weight_dict:
            a, b = pair()
            out[target] = sample(a) - sample(b)
    return out


def _reference(crit64, tensors, with_prev):
    """The fp64 module path on the CPU, after the premise that makes it a reference for the l1-ds terms: none of their differences sits
    within rounding of the kink, where the fp32 side may take the other sign."""
    for target, d in _l1_ds_differences(crit64, tensors[1].double(), tensors[2].double()).items():
        close = (d != 0) & (d.abs() < 1e-5)
        assert not close.any(), (target, d[close])
    return _run(crit64, tensors, "cpu", torch.float64, with_prev)


def _count_calls(monkeypatch, ops, name):
    calls = []
    inner = getattr(ops, name)

    def counted(*a, **k):
        calls.append(name)
        return inner(*a, **k)
    monkeypatch.setattr(ops, name, counted)
    return calls


def _compare(got, want, h, w, tensors, what):
    """The bars of test_fused_unshaded_loss_matches_module_path: values and total 1e-5 * max(1, |v|), gradients 2e-5 of the largest
    entry.  A pixel with a zero normal has a gradient of g / 1e-7, seven orders above every other entry, so the gradient of ``pred`` is
    held to the same bar a second time over the other pixels alone."""
    total, values, gpred, gprev = got
    total64, values64, gpred64, gprev64 = want
    assert set(values) == set(values64), what
    for k in values64:
        assert abs(values[k] - values64[k]) <= 1e-5 * max(1.0, abs(values64[k])), (what, k, values[k], values64[k])
    assert abs(total - total64) <= 1e-5 * max(1.0, abs(total64)), (what, total, total64)
    gpred, gpred64 = gpred.double().cpu(), gpred64.double().cpu()
    err, scale = (gpred - gpred64).abs().max().item(), gpred64.abs().max().item()
    assert scale > 0 and err <= 2e-5 * scale, (what, err, scale)
    ordinary = (tensors[1][:, 1:4].abs().sum(dim=1, keepdim=True) > 0).expand_as(gpred64)
    err, scale = ((gpred - gpred64) * ordinary).abs().max().item(), (gpred64 * ordinary).abs().max().item()
    print("%s: gradient of pred within %.2e of the largest ordinary entry %.3g" % (what, err / scale, scale))
    assert err <= 2e-5 * scale, (what, err, scale)
    if gprev64 is not None:
        gprev, gprev64 = gprev.double().cpu(), gprev64.double().cpu()
        assert (gprev - gprev64).abs().max().item() <= 2e-5 * gprev64.abs().max().item(), what


@pytest.mark.parametrize("index", range(len(ds_common.CASES)))
def test_fused_matches_the_reference(index, monkeypatch):
    from isosurfacesuperresolution_amd import ops
    calls = _count_calls(monkeypatch, ops, "loss_unshaded_ds")
    ds_common.check_case(index, "cuda")
    assert calls == ["loss_unshaded_ds"]


# (n, h, w, padding, spec, lossAO, inverse_ao, views at an odd storage offset, seed); a seed is kept where the fp64 module path alone
# satisfies the premise of _reference (the stream 14 has an l1-ds:normal difference of 8e-6 at 32 x 64, so that case draws from 16)
PARITY = [(1, 4, 4, 0, DS_ONLY, 0.5, False, False, 1), (3, 4, 4, 1, FULL, 0.0, False, False, 2),
          (1, 8, 12, 0, FULL, 0.5, True, False, 3), (3, 8, 12, 1, DS_ONLY, 0.0, False, True, 4), (1, 8, 12, 2, DS_ONLY, 0.5, False, False, 5),
          (3, 16, 16, 0, DS_ONLY, 0.5, True, False, 6), (1, 16, 16, 1, FULL, 0.5, False, False, 7), (3, 16, 16, 2, FULL, 0.0, False, True, 8),
          (1, 16, 16, 4, DS_ONLY, 0.0, True, False, 9), (3, 16, 16, 5, FULL, 0.5, False, False, 10),
          (1, 32, 64, 0, DS_ONLY, 0.0, False, True, 11), (3, 32, 64, 1, DS_ONLY, 0.5, False, False, 12), (1, 32, 64, 2, FULL, 0.0, True, False, 13),
          (1, 32, 64, 4, DS_ONLY, 0.5, True, False, 16),(3, 32, 64, 5, FULL, 0.5, False, False, 15)]


@pytest.mark.parametrize("n,h,w,padding,spec,ao,inverse_ao,odd_views,seed", PARITY)
def test_fused_matches_the_module_path_in_fp64(n, h, w, padding, spec, ao, inverse_ao, odd_views, seed, monkeypatch):
    from isosurfacesuperresolution_amd import ops
    tensors = _inputs(n, h, w, seed)
    with_prev = spec == FULL
    crit64 = _criterion("cpu", spec, h, padding, ao, inverse_ao).double()
    want = _reference(crit64, tensors, with_prev)
    calls = _count_calls(monkeypatch, ops, "loss_unshaded_ds")
    got = _run(_criterion("cuda", spec, h, padding, ao, inverse_ao), tensors, "cuda", torch.float32, with_prev, odd_views)
    assert calls == ["loss_unshaded_ds"]
    _compare(got, want, h, w, tensors, "N %d, %d x %d, padding %d" % (n, h, w, padding))
    if h >= 12 and padding <= 5:          # the cell with equal masks lies inside the border: its l1-ds:mask difference is exactly 0
        d = _l1_ds_differences(crit64, tensors[1].double(), tensors[2].double())["mask"]
        assert (d[:, 0, 2, 1] == 0).all()


def test_more_cells_than_threads_in_the_grid():
    """512 workgroups of 256 threads own 131072 cells at a time; 2 x 256 x 257 cells take a second trip through the loop.  The l2-ds
    terms alone: among half a million l1 differences some lie within rounding of 0, and the premise above cannot hold.  The fp64 module
    path runs on the GPU here."""
    n, h, w, padding = 2, 1024, 1028, 3
    assert n * (h // 4) * (w // 4) > 512 * 256
    tensors = _inputs.__wrapped__(n, h, w, 21)
    want = _run(_criterion("cuda", L2_ONLY, h, padding).double(), tensors, "cuda", torch.float64, False)
    got = _run(_criterion("cuda", L2_ONLY, h, padding), tensors, "cuda", torch.float32, False)
    _compare(got, want, h, w, tensors, "N %d, %d x %d, padding %d" % (n, h, w, padding))
    assert got[2][:, :, -8:, -8:].abs().max().item() > 0          # the last cells were reached


def _pad(img, border):
    from isosurfacesuperresolution_amd.losses import LossNetUnshaded
    return LossNetUnshaded.pad(img, border)


def _centre_mean(x):
    return 0.25 * ((x[:, :, 1::4, 1::4] + x[:, :, 1::4, 2::4]) + (x[:, :, 2::4, 1::4] + x[:, :, 2::4, 2::4]))


def test_equal_masks_give_no_l1_gradient():
    """A cell in which the prediction's mask equals the input's: ``l1-ds:mask`` differs by exactly 0 there and sgn(0) = 0."""
    gt, pred, inp, _ = _inputs(1, 16, 16, 7)
    crit = _criterion("cuda", "l1-ds:mask:1", 16, 2)
    p = pred.cuda().requires_grad_(True)
    total, values = crit(gt.cuda(), p, inp.cuda(), None, None)
    total.backward()
    assert p.grad[:, 0, 8:12, 4:8].abs().max().item() == 0.0
    assert (p.grad[:, 0, 5:7, 5:7].abs() == 1.0 / 64).all()          # an ordinary cell: weight / count (16 cells) / 4 at each centre pixel
    want = (_centre_mean(_pad(pred, 2)[:, 0:1].double()) - _centre_mean(inp[:, 0:1].double())).abs().mean().item()
    assert abs(values[("l1-ds", "mask")] - want) <= 1e-6


@pytest.mark.parametrize("padding", [0, 2, 5])
def test_gradient_structure_of_a_ds_only_criterion(padding):
    """Border pixels receive nothing; with the base terms' weights 0 the twelve non-centre pixels of every cell receive exactly 0."""
    gt, pred, inp, _ = _inputs(3, 16, 16, 6)
    crit = _criterion("cuda", DS_ONLY, 16, padding)
    p = pred.cuda().requires_grad_(True)
    total, _ = crit(gt.cuda(), p, inp.cuda(), None, None)
    (total * UPSTREAM).backward()
    g = p.grad
    centre = torch.zeros(16, 16, dtype=torch.bool, device="cuda")
    for y in (1, 2):
        for x in (1, 2):
            centre[y::4, x::4] = True
    inside = torch.zeros_like(centre)
    inside[padding:16 - padding, padding:16 - padding] = True
    if padding:
        assert g[:, :, ~inside].abs().max().item() == 0.0
    assert g[:, :, ~centre].abs().max().item() == 0.0
    unequal = torch.ones_like(centre)
    unequal[8:12, 4:8] = False                               # (the cell of _inputs in which the two masks are equal)
    assert (g[:, 0][:, centre & inside & unequal] != 0).all()          # the mask terms reach every centre pixel inside the border


def test_existing_terms_keep_their_bits():
    """``ops.loss_unshaded_ds`` with no ds term enabled: values [0..15] and both gradients are those of ``ops.loss_unshaded``."""
    from isosurfacesuperresolution_amd import ops
    gt, pred, inp, prev = (t.cuda() for t in _inputs(3, 32, 64, 12))
    crit = _criterion("cuda", ds_common.RECIPE, 32, 4, ao=0.0)
    weights = {k: v for k, v in crit.weight_dict.items() if k[0] in ops.LOSS_KINDS}
    cfg = ops.loss_unshaded_config(weights, 4, crit.shading)
    ds_cfg = ops.loss_downsample_config({}, 4, crit.shading)
    assert ds_cfg["enabled"] == 0
    out = []
    for with_ds in (False, True):
        p, v = pred.clone().requires_grad_(True), prev.clone().requires_grad_(True)
        vals = ops.loss_unshaded_ds(gt, p, v, inp, cfg, ds_cfg) if with_ds else ops.loss_unshaded(gt, p, v, cfg)
        (vals[15] * UPSTREAM).backward()
        out.append((vals.detach(), p.grad, v.grad))
    (v16, gp, gv), (v24, gp_ds, gv_ds) = out
    assert v16.shape == (16,) and v24.shape == (24,)
    assert torch.equal(v16, v24[:16]) and v24[16:].abs().max().item() == 0.0
    assert torch.equal(gp, gp_ds) and torch.equal(gv, gv_ds) and gp.abs().max().item() > 0


def test_two_calls_give_the_same_bits():
    tensors = _inputs(3, 32, 64, 15)
    crit = _criterion("cuda", FULL, 32, 5)
    first = _run(crit, tensors, "cuda", torch.float32, True)
    second = _run(crit, tensors, "cuda", torch.float32, True)
    assert first[0] == second[0] and first[1] == second[1]
    assert torch.equal(first[2], second[2]) and torch.equal(first[3], second[3])


@pytest.mark.parametrize("h,w", [(6, 8), (8, 6)])
def test_other_sizes_take_the_module_path(h, w, monkeypatch):
    from isosurfacesuperresolution_amd import ops
    tensors = _inputs(2, h, w, 31)
    want = _reference(_criterion("cpu", FULL, h, 1).double(), tensors, True)
    calls_ds, calls_plain = _count_calls(monkeypatch, ops, "loss_unshaded_ds"), _count_calls(monkeypatch, ops, "loss_unshaded")
    got = _run(_criterion("cuda", FULL, h, 1), tensors, "cuda", torch.float32, True)
    assert calls_ds == [] and calls_plain == [] and not ops.loss_downsample_supported(tensors[1].cuda(), tensors[2].cuda(), 1)
    _compare(got, want, h, w, tensors, "%d x %d" % (h, w))


def test_an_input_that_needs_a_gradient_takes_the_module_path():
    from isosurfacesuperresolution_amd import ops
    gt, pred, inp, _ = (t.cuda() for t in _inputs(1, 16, 16, 7))
    assert ops.loss_downsample_supported(pred, inp, 2) and not ops.loss_downsample_supported(pred, inp.clone().requires_grad_(True), 2)
    assert not ops.loss_downsample_supported(pred, inp.double(), 2) and not ops.loss_downsample_supported(pred, inp[:, :4], 2)
    assert not ops.loss_downsample_supported(pred, inp, 8) and not ops.loss_downsample_supported(pred.cpu(), inp.cpu(), 2)
    crit = _criterion("cuda", DS_ONLY, 16, 2)
    i = inp.clone().requires_grad_(True)
    total, _ = crit(gt, pred, i, None, None)
    total.backward()
    assert i.grad is not None and i.grad.abs().max().item() > 0


def test_fused_off_agrees_with_fused_on():
    tensors = _inputs(3, 16, 16, 10)          # (the premise for these inputs is asserted by the parity case with seed 10)
    crit = _criterion("cuda", FULL, 16, 5)
    on = _run(crit, tensors, "cuda", torch.float32, True)
    crit.fused = False
    off = _run(crit, tensors, "cuda", torch.float32, True)
    _compare(on, off, 16, 16, tensors, "fused on / off")


def test_c_abi_refuses_what_it_cannot_run():
    from isosurfacesuperresolution_amd import ops
    lib = ops._sr()
    assert lib.isrLossDownsampleSupported(2, 16, 16, 2) == 1 and lib.isrLossDownsampleSupported(2, 16, 14, 2) == 0
    assert lib.isrLossDownsampleSupported(2, 6, 16, 2) == 0 and lib.isrLossDownsampleSupported(2, 16, 16, 8) == 0
    assert lib.isrLossDownsampleSupported(1, 4, 4, 1) == 1 and lib.isrLossDownsampleSupported(1, 4, 4, 2) == 0
    crit = _criterion("cuda", DS_ONLY, 16, 2)
    cfg = ops.loss_downsample_config(crit.weight_dict, 2, crit.shading)
    assert cfg["enabled"] == 0xff
    pred, inp = torch.zeros(2 * 6 * 256 + 1, device="cuda"), torch.zeros(2 * 5 * 256 + 1, device="cuda")
    ws = torch.zeros(lib.isrLossDownsampleWorkspace() // 4, device="cuda")
    values = torch.full((9,), 7.0, device="cuda")

    def forward(p, i, h=16):
        return lib.isrLossDownsampleForward(ops._ptr(p), ops._ptr(i), 2, h, 16, 2, cfg["weights"], cfg["enabled"], cfg["shading"], cfg["ao"],
                                            cfg["inverse_ao"], ops._ptr(ws), ops._ptr(values), ops._offset_ptr(values, 8), ops._stream())
    assert forward(pred[1:], inp) == -1 and forward(pred, inp[1:]) == -1 and forward(pred, inp, h=14) == -1
    gpred = torch.full((2 * 6 * 256 + 1,), 7.0, device="cuda")
    assert lib.isrLossDownsampleBackward(ops._ptr(pred), ops._ptr(inp), 2, 16, 16, 2, cfg["weights"], cfg["enabled"], cfg["shading"], cfg["ao"],
                                         cfg["inverse_ao"], ops._ptr(values), ops._ptr(gpred[1:]), ops._stream()) == -1
    torch.cuda.synchronize()
    assert (values == 7.0).all() and (gpred == 7.0).all()          # nothing was launched
    assert forward(pred, inp) == 0
    torch.cuda.synchronize()
    assert values[8].item() != 7.0


def test_one_captured_step():
    """``train.GraphedTrainStep`` with ds terms in the criterion captures and replays; replay k gives the loss of the eager step k
    (1e-5 relative, the bar of test_bn_model_gpu's eager / graphed pair; plain SGD for the reason given there)."""
    from isosurfacesuperresolution_amd import losses, models, train
    opt = ds_common.options(ds_common.RECIPE + ",l1-ds:normal:1,l2-ds:color:1", ao=0.0, reconType='residual', useBN=False, numResidualLayers=2)
    rs = np.random.RandomState(41)
    inp = torch.from_numpy(rs.uniform(0, 1, (2, 3, 5, 8, 8)).astype(np.float32)).cuda()
    inp[:, :, 0] = inp[:, :, 0] * 2 - 1
    flow = torch.from_numpy(rs.uniform(-0.025, 0.025, (2, 3, 2, 8, 8)).astype(np.float32)).cuda()
    tgt = torch.from_numpy(rs.uniform(0, 1, (2, 3, 6, 32, 32)).astype(np.float32)).cuda()
    tgt[:, :, 0] = tgt[:, :, 0] * 2 - 1
    batch = (inp, flow, tgt)
    crit = losses.LossNetUnshaded("cuda", 5, 6, 32, 4, opt).cuda()
    assert crit.uses_input and not crit.uses_previous_input
    nets = []
    for _ in range(2):
        torch.manual_seed(11)
        nets.append(models.createNetwork('EnhanceNet', 4, 101, [0, 1, 2, 3, 4], 6, opt).cuda().train())
    eager_net, graph_net = nets
    eager_opt, graph_opt = (torch.optim.SGD(net.parameters(), lr=1e-3) for net in nets)
    step = train.GraphedTrainStep(graph_net, crit, graph_opt, batch, warmup=3, initial_image="zero")
    for k in range(2):
        eager_loss = train.train_step(eager_net, crit, eager_opt, batch, initial_image="zero")
        graph_loss = float(step(batch))
        torch.cuda.synchronize()
        print("step %d: eager %.6f graphed %.6f" % (k, eager_loss, graph_loss))
        assert abs(graph_loss - eager_loss) <= 1e-5 * max(1.0, abs(eager_loss)), (k, graph_loss, eager_loss)
