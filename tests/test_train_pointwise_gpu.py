"""The element-wise and warp kernels of a training step (csrc/sr_train.hip) on the device, every launch form, against the torch
composition each replaces in fp64 (train_pointwise_common): the fused loss, the recurrent input forward and backward, the x2
upsampling, the residual reconstruction, the activation backward with the phase-major gradient, and Adam.

The rule is ``discr_input_common.compare``'s: per pixel set |kernel - fp64| <= max(4 x |the same composition in fp32 - fp64|, floor),
floor 1e-6 for values and 1e-5 x the set's largest |fp64| for gradients; planted kink pixels, structural sets (tile seams, image
edges) and the rest are separate sets, border pixels are exactly 0, no pixel is left out.  The references are computed on the CPU;
the one case per capped grid that crosses its cap (``train_pointwise_common.CAPS``) evaluates the same composition in fp64 and fp32 on
the device.  Where the kernel is selects and one multiply (activation backward, phase gradient), or a claim of the design says so
(the warp's sample positions, the quad forms of the upsampling, aligned against unaligned operands), the assertion is bit equality.
Rows go to the file ISR_TRAIN_POINTWISE_REPORT names (profiles/train_pointwise_errors.md)."""
import pytest
import torch
import torch.nn.functional as F

import train_pointwise_common as P
from discr_input_common import CLEAR, compare, kink_clearance, pixel_sets
from isosurfacesuperresolution_amd import ops

pytestmark = pytest.mark.gpu


def offset_view(t):
    """The same values in a contiguous view four bytes past a 16-byte boundary (what ``.contiguous()`` keeps as it is)."""
    room = torch.zeros(t.numel() + 4, device=t.device, dtype=t.dtype)
    v = room[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def scalar_rule(case, kind, got, ref64, ref32, floor, bad):
    err, own = abs(got - ref64), abs(ref32 - ref64)
    bar = max(4.0 * own, floor)
    print("%-44s %-18s error %.3e  fp32-vs-fp64 %.3e  bar %.3e" % (case, kind, err, own, bar))
    P.record_error(case, kind, err, own, bar)
    if not err <= bar:
        bad.append((case, kind, err, bar))


# =====================================================================================================================================
# Loss
# =====================================================================================================================================
def run_loss_device(gt, pred, prev, prev_mode, losses, ao, inverse_ao, pad, views=False):
    crit = P.loss_criterion("cuda", losses, ao, inverse_ao, gt.shape[2], pad, fused=True)
    place = (lambda t: offset_view(t.cuda())) if views else (lambda t: t.cuda())
    g, p = place(gt), place(pred).requires_grad_(True)
    v = None if prev_mode == "absent" else place(prev).requires_grad_(prev_mode == "gradient")
    assert crit._fusable(g, p, v)
    total, values = crit(g, p, None, None, v)
    (total * P.UPSTREAM).backward()
    assert v is None or (v.grad is not None) == (prev_mode == "gradient")
    return values, float(total.detach()), p.grad.cpu(), v.grad.cpu() if v is not None and v.grad is not None else None


def check_loss(shape, name, variants, prev_modes, reference_device="cpu"):
    n, h, w, pad = shape
    losses = P.CONFIGURATIONS[name]
    (gt, pred, prev), planted = P.loss_operands(n, h, w, pad)
    sets, border = pixel_sets(planted, n, h, w, pad)
    bad = []
    for ao, inverse in variants:
        for x in (pred, prev):
            assert kink_clearance(x, sets["rest"], True, ao, inverse) >= CLEAR
        assert P.l1_clearance(pred, gt, sets["rest"], ao, inverse) >= CLEAR
        for mode in prev_modes:
            ref64 = P.loss_module_path(gt, pred, prev, mode, losses, ao, inverse, pad, torch.float64, reference_device)
            ref32 = P.loss_module_path(gt, pred, prev, mode, losses, ao, inverse, pad, torch.float32, reference_device)
            got = run_loss_device(gt, pred, prev, mode, losses, ao, inverse, pad)
            again = run_loss_device(gt, pred, prev, mode, losses, ao, inverse, pad)
            assert got[0] == again[0] and got[1] == again[1] and torch.equal(got[2], again[2])          # no atomics: the same bits
            assert (got[3] is None and again[3] is None) or torch.equal(got[3], again[3])
            case = "loss %dx%dx%d pad %d %s ao %.2f inv %d prev %s" % (n, h, w, pad, name, ao, inverse, mode)
            assert set(got[0]) >= set(ref64[0]) and (name != "everything" or len(ref64[0]) == (10 if mode == "absent" else 15))
            for key in sorted(got[0]):
                if key in ref64[0]:
                    scalar_rule(case, "%s:%s" % key, got[0][key], ref64[0][key], ref32[0][key], 1e-6, bad)
                else:
                    assert key[0] == "temp-l2" and mode == "absent" and got[0][key] == 0.0
            scalar_rule(case, "total", got[1], ref64[1], ref32[1], 1e-6, bad)
            bad += compare(case + " d/d pred", got[2], ref64[2], ref32[2], sets, border, True, 1e-5, P.record_error)
            assert (got[3] is None) == (mode != "gradient")
            if got[3] is not None:
                bad += compare(case + " d/d prev", got[3], ref64[3], ref32[3], sets, border, True, 1e-5, P.record_error)
    assert not bad, bad


@pytest.mark.parametrize("name", list(P.CONFIGURATIONS))
@pytest.mark.parametrize("shape", P.LOSS_SHAPES, ids=lambda s: "%dx%dx%d_pad%d" % s)
def test_loss_against_the_fp64_module_path(shape, name):
    check_loss(shape, name, P.AO_VARIANTS, P.PREV_MODES)


def test_loss_beyond_the_grid_cap():
    """270 848 quads against 1024 workgroups x 256: the stride loop of both kernels runs a second time in 8 704 threads; the partial sums of
    1024 workgroups go through the finalize kernel."""
    n, h, w, _ = P.LOSS_CAP_SHAPE
    assert P.crosses_cap("loss", n * h * (w // 4))
    check_loss(P.LOSS_CAP_SHAPE, "everything", [(0.35, True)], ["gradient"], reference_device="cuda")


def test_loss_entry_points_refuse_operands_that_are_not_16_byte_aligned():
    """By return code: nothing is launched (the workspace, the values and the gradients keep their sentinels)."""
    n, h, w, pad = P.LOSS_SHAPES[0]
    (gt, pred, prev), _ = P.loss_operands(n, h, w, pad)
    gt, pred, prev = gt.cuda(), pred.cuda(), prev.cuda()
    crit = P.loss_criterion("cuda", P.EVERYTHING, 0.35, False, h, pad, fused=True)
    cfg = ops.loss_unshaded_config({k: v for k, v in crit.weight_dict.items() if k[0] in ops.LOSS_KINDS}, pad, crit.shading)
    lib = ops._sr()
    ws = torch.full((lib.isrLossUnshadedWorkspace() // 4,), 7.0, device="cuda")
    values, gvalues = torch.full((16,), 7.0, device="cuda"), torch.ones(16, device="cuda")
    gpred, gprev = torch.full_like(pred, 7.0), torch.full_like(prev, 7.0)
    tail = (n, h, w, cfg['pad'], cfg['weights'], cfg['enabled'], cfg['shading'], cfg['ao'], cfg['inverse_ao'])

    def forward(a, b, c):
        return lib.isrLossUnshadedForward(ops._ptr(a), ops._ptr(b), ops._ptr(c), *tail, ops._ptr(ws), ops._ptr(values), ops._stream())

    def backward(a, b, c, ga, gb):
        return lib.isrLossUnshadedBackward(ops._ptr(a), ops._ptr(b), ops._ptr(c), *tail, ops._ptr(gvalues), ops._ptr(ga), ops._ptr(gb), ops._stream())

    for k in range(3):
        operands = [gt, pred, prev]
        operands[k] = offset_view(operands[k])
        assert forward(*operands) == -1 and backward(*operands, gpred, gprev) == -1
    assert backward(gt, pred, prev, offset_view(gpred), gprev) == -1 and backward(gt, pred, prev, gpred, offset_view(gprev)) == -1
    torch.cuda.synchronize()
    for t in (ws, values, gpred, gprev):
        assert bool(t.eq(7.0).all())
    assert forward(gt, pred, prev) == 0 and backward(gt, pred, prev, gpred, gprev) == 0 and forward(gt, pred, None) == 0
    torch.cuda.synchronize()
    assert not bool(gpred.eq(7.0).any())


def test_loss_of_offset_views_equals_the_aligned_result():
    """``ops.loss_unshaded`` realigns a contiguous view at an odd storage offset with a copy: the same bits as the aligned tensors."""
    n, h, w, pad = P.LOSS_SHAPES[0]
    (gt, pred, prev), _ = P.loss_operands(n, h, w, pad)
    for mode in ("gradient", "absent"):
        aligned = run_loss_device(gt, pred, prev, mode, P.EVERYTHING, 0.35, True, pad)
        views = run_loss_device(gt, pred, prev, mode, P.EVERYTHING, 0.35, True, pad, views=True)
        assert aligned[0] == views[0] and aligned[1] == views[1] and torch.equal(aligned[2], views[2])
        assert (aligned[3] is None and views[3] is None) or torch.equal(aligned[3], views[3])


# =====================================================================================================================================
# Recurrent input
# =====================================================================================================================================
def ring_sets(b, H, W):
    ring = torch.zeros(b, H, W, dtype=torch.bool)
    ring[:, 0] = ring[:, -1] = True
    ring[:, :, 0] = ring[:, :, -1] = True
    return {"outer ring": ring, "rest": ~ring}


@pytest.mark.parametrize("regime", P.FLOW_REGIMES)
@pytest.mark.parametrize("shape", P.RECURRENT_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_recurrent_input_forward(shape, regime):
    b, h, w = shape
    H, W = 4 * h, 4 * w
    (raw, clip_in, clip_flow, _, _), _ = P.recurrent_operands(b, h, w, regime)
    inp, flow = P.frames(clip_in, clip_flow)
    dev_in, dev_flow = P.frames(clip_in.cuda(), clip_flow.cuda())
    assert b == 1 or not dev_in.is_contiguous()
    netin, warped = ops.recurrent_input(raw.cuda(), dev_in, dev_flow)
    netin2, warped2 = ops.recurrent_input(raw.cuda(), dev_in, dev_flow)
    assert torch.equal(netin, netin2) and torch.equal(warped, warped2)
    from isosurfacesuperresolution_amd.models import VideoTools
    assert torch.equal(netin[:, 0:5], dev_in)
    assert torch.equal(netin[:, 5:], VideoTools.flatten_high(warped, 4))
    netin, warped = netin.cpu(), warped.cpu()
    n64, w64, _ = P.recurrent_definition(raw, inp, flow, torch.float64)
    n32, w32, _ = P.recurrent_definition(raw, inp, flow, torch.float32)
    case = "recurrent forward %dx%dx%d %s" % (b, h, w, regime)
    bad = compare(case + " warped", warped, w64, w32, ring_sets(b, H, W), P.no_border(b, H, W), False, 1e-6, P.record_error)
    bad += compare(case + " net input", netin, n64, n32, {"all": ~P.no_border(b, h, w)}, P.no_border(b, h, w), False, 1e-6, P.record_error)
    assert not bad, bad
    # a sample more than a pixel outside the image reads nothing: mask exactly -1, the other channels exactly 0
    sx, sy = P.sample_positions(flow)
    outside = (sx < -1.001) | (sx > W + 0.001) | (sy < -1.001) | (sy > H + 0.001)
    assert bool(outside.any()) or regime != "far"
    far = warped.permute(0, 2, 3, 1)[outside]
    assert bool((far[:, 0] == -1.0).all()) and not far[:, 1:].any()


@pytest.mark.parametrize("regime", P.FLOW_REGIMES)
@pytest.mark.parametrize("shape", P.RECURRENT_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_recurrent_input_samples_at_the_module_paths_positions_bit_for_bit(shape, regime):
    """csrc/sr_warp_exact.h and models/videotools.py fix the operations of the sample position and of the blend so that kernel and fp32
    module path agree bit for bit.  ``warped`` against ``VideoTools.warp_upscale`` in fp32 on the CPU: mask, depth and ao pass clamps and
    the contraction-free blend only and must be EQUAL; the normal channels differ by the roundings of |n| (WARPED_NORMAL_BAR, derived
    in train_pointwise_common).  Against fp64 the module path itself is 1e-5 to 7e-5 away at this width (position rounding times the
    image's slope), so the 4 x rule of the forward test alone would not see a position that is one bit off."""
    b, h, w = shape
    (raw, clip_in, clip_flow, _, _), _ = P.recurrent_operands(b, h, w, regime)
    inp, flow = P.frames(clip_in, clip_flow)
    dev_in, dev_flow = P.frames(clip_in.cuda(), clip_flow.cuda())
    _, warped = ops.recurrent_input(raw.cuda(), dev_in, dev_flow)
    _, w32, _ = P.recurrent_definition(raw, inp, flow, torch.float32)
    diff = (warped.cpu().double() - w32).abs().amax(dim=(0, 2, 3))
    print("warped - fp32 module path, per channel:", ["%.3e" % float(d) for d in diff])
    for c, d in enumerate(diff):
        P.record_error("recurrent forward %dx%dx%d %s warped vs fp32 module path" % (b, h, w, regime), "channel %d" % c, float(d), 0.0,
                       P.WARPED_NORMAL_BAR if c in (1, 2, 3) else 0.0)
    for c in (0, 4, 5):
        assert torch.equal(warped[:, c].cpu().double(), w32[:, c]), (c, float(diff[c]))
    assert float(diff[1:4].max()) <= P.WARPED_NORMAL_BAR


def run_recurrent_backward(raw, dev_in, dev_flow, gn, gw, through_autograd):
    """d / d raw: through ``ops.recurrent_input`` under autograd (both upstreams), or from the entry point itself with the upstream that
    is absent passed as NULL."""
    r = raw.cuda()
    if through_autograd:
        r.requires_grad_(True)
        netin, warped = ops.recurrent_input(r, dev_in, dev_flow)
        ((netin * gn.cuda()).sum() + (warped * gw.cuda()).sum()).backward()
        return r.grad.cpu()
    b, _, H, W = r.shape
    flo, fstride = ops._batch_view(dev_flow, 2, H // 4, W // 4)
    g_netin, g_warped = gn.cuda() if gn is not None else None, gw.cuda() if gw is not None else None
    scratch, g_raw = torch.empty_like(r), torch.empty_like(r)
    rc = ops._sr().isrRecurrentInputBackward(ops._ptr(r), ops._ptr(flo), ops._ptr(g_netin), ops._ptr(g_warped), ops._ptr(scratch), ops._ptr(g_raw),
                                             b, H // 4, W // 4, fstride, ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    return g_raw.cpu()


def check_recurrent_backward(shape, regime, modes, reference_device="cpu"):
    b, h, w = shape
    H, W = 4 * h, 4 * w
    (raw, clip_in, clip_flow, gn, gw), planted = P.recurrent_operands(b, h, w, regime)
    inp, flow = P.frames(clip_in, clip_flow)
    dev_in, dev_flow = P.frames(clip_in.cuda(), clip_flow.cuda())
    sets = P.recurrent_sets(planted, b, H, W)
    unplanted = sets["rest"] | sets["seam in X"] | sets["seam in Y"] | sets["outer ring"]
    assert P.raw_clearance(raw, unplanted) >= CLEAR
    bad = []
    for mode in modes:
        a, c = (gn if mode != "g_warped only" else None), (gw if mode != "g_netin only" else None)
        _, _, ref64 = P.recurrent_definition(raw, inp, flow, torch.float64, reference_device, g_netin=a, g_warped=c)
        _, _, ref32 = P.recurrent_definition(raw, inp, flow, torch.float32, reference_device, g_netin=a, g_warped=c)
        got = run_recurrent_backward(raw, dev_in, dev_flow, a, c, through_autograd=(mode == "both"))
        case = "recurrent backward %dx%dx%d %s %s" % (b, h, w, regime, mode)
        bad += compare(case, got, ref64, ref32, sets, P.no_border(b, H, W), True, 1e-5, P.record_error)
    assert not bad, bad


@pytest.mark.parametrize("regime", P.FLOW_REGIMES)
@pytest.mark.parametrize("shape", P.RECURRENT_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_recurrent_input_backward(shape, regime):
    """(2, 5, 66): five tile columns of the scatter, the last 8 pixels wide, and two tile rows, the last 4 high; 'near' flows keep every tap
    in the LDS window and cross the seams both ways, 'far' ones take the direct-to-memory path and leave the image."""
    check_recurrent_backward(shape, regime, ("both", "g_netin only", "g_warped only"))


def test_recurrent_input_backward_beyond_the_grid_caps():
    b, h, w = P.RECURRENT_CAP_SHAPE
    assert P.crosses_cap("recurrent_post", 16 * b * h * w) and P.crosses_cap("recurrent_fill", 16 * b * h * w * 6 // 4)
    check_recurrent_backward(P.RECURRENT_CAP_SHAPE, "near", ("both",), reference_device="cuda")


# =====================================================================================================================================
# x2 upsampling
# =====================================================================================================================================
def check_upsample(case, x, gy, forward, backward, reference_device="cpu"):
    n, c, h, w = x.shape
    y64, g64 = P.upsample_definition(x, gy, torch.float64, reference_device)
    y32, g32 = P.upsample_definition(x, gy, torch.float32, reference_device)
    bad = []
    if forward is not None:
        bad += compare(case + " values", forward, y64, y32, P.edge_sets(n, 2 * h, 2 * w), P.no_border(n, 2 * h, 2 * w), False, 1e-6, P.record_error)
    if backward is not None:
        bad += compare(case + " gradient", backward, g64, g32, P.edge_sets(n, h, w), P.no_border(n, h, w), True, 1e-5, P.record_error)
    assert not bad, bad


def upsample_entry(x, gy):
    """(y, gx) from the entry points themselves, at whatever addresses ``x`` and ``gy`` have (outputs aligned)."""
    n, c, h, w = x.shape
    lib = ops._sr()
    y, gx = torch.empty(n, c, 2 * h, 2 * w, device="cuda"), torch.empty(n, c, h, w, device="cuda")
    assert lib.isrUpsample2xForward(ops._ptr(x), ops._ptr(y), n * c, h, w, ops._stream()) == 0
    assert lib.isrUpsample2xBackward(ops._ptr(gy), ops._ptr(gx), n * c, h, w, ops._stream()) == 0
    torch.cuda.synchronize()
    return y, gx


@pytest.mark.parametrize("shape", P.UPSAMPLE_SHAPES, ids=str)
def test_upsample2x_against_fp64(shape):
    """w % 4 == 0: the quad kernels (upsample2x_fwd4 / bwd4); w even: the generic <4> forward; w odd: the generic <2> forward; both of
    the latter the generic backward.  For w % 4 == 0 the same data through views four bytes off a 16-byte boundary: ``x`` there takes
    the generic <4> forward and ``gy`` the generic backward (these launches are not in the profiler's records: the dispatch rule of
    isrUpsample2xForward / Backward -- quad kernels only where both pointers are 16-byte aligned -- is the evidence for the route), and
    the header's promise is that every form gives the same bits."""
    n, c, h, w = shape
    x, gy = P.uniform(31, *shape), P.uniform(32, n, c, 2 * h, 2 * w)
    xd = x.cuda().requires_grad_(True)
    y = ops.bilinear_upsample2x(xd)
    y.backward(gy.cuda())
    check_upsample("upsample %s" % (shape,), x, gy, y.detach().cpu(), xd.grad.cpu())
    y_entry, gx_entry = upsample_entry(x.cuda(), gy.cuda())
    assert torch.equal(y_entry, y.detach()) and torch.equal(gx_entry, xd.grad)
    if w % 4 == 0:
        y_off, gx_off = upsample_entry(offset_view(x.cuda()), offset_view(gy.cuda()))
        assert torch.equal(y_off, y.detach()), float((y_off - y.detach()).abs().max())
        assert torch.equal(gx_off, xd.grad), float((gx_off - xd.grad).abs().max())


def test_upsample2x_beyond_the_grid_caps():
    n, c, h, w = P.UPSAMPLE_CAP_FORWARD
    assert P.crosses_cap("upsample_forward", n * c * 2 * h * (2 * w // 4))
    x = P.uniform(33, n, c, h, w)
    y = ops.bilinear_upsample2x(x.cuda())
    check_upsample("upsample forward cap %s" % (P.UPSAMPLE_CAP_FORWARD,), x, torch.zeros(n, c, 2 * h, 2 * w), y.cpu(), None, "cuda")
    n, c, h, w = P.UPSAMPLE_CAP_BACKWARD
    assert P.crosses_cap("upsample_backward", n * c * h * w)
    gy = P.uniform(34, n, c, 2 * h, 2 * w)
    gx = torch.empty(n, c, h, w, device="cuda")
    assert ops._sr().isrUpsample2xBackward(ops._ptr(gy.cuda()), ops._ptr(gx), n * c, h, w, ops._stream()) == 0
    torch.cuda.synchronize()
    check_upsample("upsample backward cap %s" % (P.UPSAMPLE_CAP_BACKWARD,), torch.zeros(n, c, h, w), gy, None, gx.cpu(), "cuda")


# =====================================================================================================================================
# Residual reconstruction
# =====================================================================================================================================
def check_recon(shape, reference_device="cpu"):
    n, cout, cin, k, h, w = shape
    y, x, g = P.uniform(41, n, cout, 4 * h, 4 * w), P.uniform(42, n, cin, h, w), P.uniform(43, n, cout, 4 * h, 4 * w)
    yd, xd = y.cuda().requires_grad_(True), x.cuda().requires_grad_(True)
    assert ops.recon_residual_supported(yd, xd, k)
    out = ops.recon_residual(yd, xd, k)
    out.backward(g.cuda())
    o64, gy64, gx64 = P.recon_definition(y, x, k, g, torch.float64, reference_device)
    o32, gy32, gx32 = P.recon_definition(y, x, k, g, torch.float32, reference_device)
    case = "recon %s" % (shape,)
    bad = compare(case + " values", out.detach().cpu(), o64, o32, P.edge_sets(n, 4 * h, 4 * w), P.no_border(n, 4 * h, 4 * w), False, 1e-6, P.record_error)
    bad += compare(case + " d/d x", xd.grad.cpu(), gx64, gx32, P.edge_sets(n, h, w), P.no_border(n, h, w), True, 1e-5, P.record_error)
    assert not bad, bad
    assert torch.equal(yd.grad.cpu(), g)                                    # the network output's gradient is the upstream, untouched
    assert not xd.grad[:, k:].any() and not gx64[:, k:].any()               # channels the reconstruction does not read: exactly 0
    assert torch.equal(out.detach()[:, k:], yd.detach()[:, k:])
    xd2 = x.cuda().requires_grad_(True)
    ops.recon_residual(y.cuda(), xd2, k).backward(g.cuda())
    assert torch.equal(xd2.grad, xd.grad)


@pytest.mark.parametrize("shape", P.RECON_SHAPES, ids=str)
def test_residual_reconstruction_against_fp64(shape):
    """(.., 3, 65): 4 w = 260 puts four live threads in the forward's second workgroup in X."""
    check_recon(shape)


def test_residual_reconstruction_beyond_the_fills_cap():
    n, cout, cin, k, h, w = P.RECON_CAP_SHAPE
    assert P.crosses_cap("recon_fill", n * cin * h * w)
    check_recon(P.RECON_CAP_SHAPE, reference_device="cuda")


# =====================================================================================================================================
# Activation backward, phase-major gradient: selects and one multiply -> the fp32 rule's bits
# =====================================================================================================================================
def act_entry(gy, y, act):
    gz = torch.full_like(gy, 7.0)
    rc = ops._sr().isrActBackward(ops._ptr(gy), ops._ptr(y), ops._ptr(gz), gy.numel(), ops.ACT_CODES[act], P.SLOPE, ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    return gz


@pytest.mark.parametrize("act", P.ACTS)
@pytest.mark.parametrize("count", P.ACT_COUNTS + [P.ACT_CAP_COUNT])
def test_act_backward_is_the_rule_bit_for_bit(count, act):
    """Counts with every ``count % 4`` tail, one beyond 2048 workgroups x 1024 elements; aligned pointers (16-byte accesses) and the same
    data four bytes off (the dword form): the same bits."""
    assert P.crosses_cap("act_backward", count) == (count == P.ACT_CAP_COUNT)
    gy, y = P.act_operands(count, count)
    want = P.act_backward_rule(gy, y, act, P.SLOPE)
    got = act_entry(gy.cuda(), y.cuda(), act)
    assert torch.equal(got.cpu(), want)
    if act != "none":
        closed = ~(y > 0)
        assert bool((y == 0).any()) and torch.equal(got.cpu()[closed], gy[closed] * (0.0 if act == "relu" else P.SLOPE))
    room = torch.full((count + 8,), 7.0, device="cuda")                     # the output four bytes off too: nothing beyond it is written
    gz = room[1:1 + count]
    assert gz.data_ptr() % 16 == 4
    gy_off, y_off = offset_view(gy.cuda()), offset_view(y.cuda())
    rc = ops._sr().isrActBackward(ops._ptr(gy_off), ops._ptr(y_off), ops._ptr(gz), count, ops.ACT_CODES[act], P.SLOPE, ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(gz.cpu(), want) and bool(room[0] == 7.0) and bool(room[1 + count:].eq(7.0).all())


@pytest.mark.parametrize("act", P.ACTS)
@pytest.mark.parametrize("shape", [(1, 1, 1, c) for c in P.ACT_COUNTS] + [(2, 3, 3, 5), P.PHASE_CAP_SHAPE], ids=str)
def test_phase_gradient_is_the_rule_bit_for_bit(shape, act):
    n, c, h, w = shape
    assert P.crosses_cap("phase_gradient", n * c * h * w) == (shape == P.PHASE_CAP_SHAPE)
    gy, y = P.act_operands(n * c * h * w, n * c * 4 * h * w)
    gy, y = gy.view(n, c, 2 * h, 2 * w), y.view(n, c, 2 * h, 2 * w)
    want = P.phase_gradient_rule(gy, y, act, P.SLOPE)
    got = ops.conv_transpose_phase_gradient(gy.cuda(), None if act == "none" else y.cuda(), act, P.SLOPE)
    assert got.shape == (n, 4 * c, h, w) and torch.equal(got.cpu(), want)
    if shape != P.PHASE_CAP_SHAPE:                                          # the dword form (planes that are not 8-byte aligned)
        got = ops.conv_transpose_phase_gradient(offset_view(gy.cuda()), None if act == "none" else offset_view(y.cuda()), act, P.SLOPE)
        assert torch.equal(got.cpu(), want)


# =====================================================================================================================================
# Adam
# =====================================================================================================================================
@pytest.mark.parametrize("first_step", [0, 1000])
@pytest.mark.parametrize("n", P.ADAM_SIZES)
def test_adam_against_float64_adam(n, first_step):
    """Five steps with a changing learning rate against float64 Adam with Python-double bias corrections: the update p_new - p_old of every
    step relative to lr, the moments after the last step relative per element; bars four times torch.optim.Adam's own fp32 distance,
    not below the floors derived in train_pointwise_common.  The learning rate as a float and as a device tensor: the same bits.
    n = 1 049 353 is beyond 4096 workgroups x 256; ``first_step`` 1000 sets the optimizer's state (no loop)."""
    assert P.crosses_cap("adam", n) == (n == P.ADAM_SIZES[1])
    lrs = P.ADAM_LRS
    grads = P.adam_gradients(n, n, len(lrs))
    p0, m0, v0 = P.adam_state(n, n, warm=first_step > 0)
    u64, m64, v64 = P.adam_reference(torch.float64, p0, m0, v0, grads, lrs, first_step)
    u32, m32, v32 = P.adam_reference(torch.float32, p0, m0, v0, grads, lrs, first_step)
    runs = []
    for as_tensor in (False, True):
        p, m, v = p0.cuda(), m0.cuda(), v0.cuda()
        step = torch.tensor([float(first_step)], device="cuda")
        lr_of = (lambda lr: torch.tensor([lr], dtype=torch.float32, device="cuda")) if as_tensor else (lambda lr: lr)
        runs.append(P.adam_trajectory(lambda p, g, m, v, k, lr: ops.adam_flat_step(p, g.cuda(), m, v, step, lr_of(lr), P.BETA1, P.BETA2, P.EPS),
                                      p, m, v, grads, lrs))
        assert float(step) == first_step + len(lrs)
    (ud, md, vd), (ut, mt, vt) = runs
    assert torch.equal(md, mt) and torch.equal(vd, vt) and all(torch.equal(a, b) for a, b in zip(ud, ut))
    case = "adam n %d from step %d" % (n, first_step)
    bad = []

    def rule(kind, err, own, floor):
        bar = max(4.0 * own, floor)
        print("%-32s %-22s error %.3e  fp32-vs-fp64 %.3e  bar %.3e" % (case, kind, err, own, bar))
        P.record_error(case, kind, err, own, bar)
        if not err <= bar:
            bad.append((case, kind, err, bar))

    largest_p = float(p0.abs().max())
    for k, lr in enumerate(lrs):
        largest_p += float(u64[k].abs().max())
        assert not ud[k][:128].any()                                        # zero gradients, zero moments: the parameter does not move
        floor = P.ADAM_FLOOR_UPDATE * float((u64[k] / lr).abs().max()) + P.U * largest_p / lr
        rule("update / lr, step %d" % (first_step + k + 1), float(((ud[k] - u64[k]) / lr).abs().max()), float(((u32[k] - u64[k]) / lr).abs().max()), floor)
    rule("exp_avg", P.relative_error(md, m64), P.relative_error(m32, m64), P.ADAM_FLOOR_M)
    rule("exp_avg_sq", P.relative_error(vd, v64), P.relative_error(v32, v64), P.ADAM_FLOOR_V)
    assert not bad, bad
