"""What tests/test_train_pointwise_cpu.py and tests/test_train_pointwise_gpu.py share: the element-wise and warp kernels of a training
step (csrc/sr_train.hip: loss, recurrent input, x2 upsampling, residual reconstruction, activation backward, Adam), each written as the
torch composition it replaces and callable in any float type, operands whose kinks are under control, the pixel sets of the
comparison, and the grid caps of the entry points.  Nothing here needs a device.

The comparison rule is ``discr_input_common.compare``: per pixel set |kernel - fp64| <= max(4 x |the same composition in fp32 - fp64|,
floor), floor 1e-6 for values and 1e-5 x the set's largest |fp64| for gradients, border pixels exactly 0, no pixel left out.

Kinks.  The loss has those of the shader (``discr_input_common``) and one family more: each of the nine field differences
``pred - gt`` against 0, where l1's derivative jumps.  ``loss_operands`` MOVES (redraws) every interior pixel of ``pred`` where a
difference that is not exactly 0 comes within ``CLEAR`` of 0; a difference that is exactly 0 (both sides gated or clamped to the same
number) is the same 0 in every precision and stays.  The raw prediction of the recurrent input has the clamps of mask (-1, 1), depth
and ao (0, 1) and ``normalize``'s 1e-7.  The warp has none: a bilinear sample with zero padding is continuous in its position."""
import argparse
import os

import numpy as np
import torch
import torch.nn.functional as F

from discr_input_common import CLEAR, TINY, compare, field6, kink_clearance, pixel_sets, plant      # noqa: F401  (re-exported)

U = 2.0 ** -24                       # unit roundoff of fp32

# ---- grid caps of the entry points (csrc/sr_train.hip): name -> (most workgroups, work items one pass of a workgroup takes) ----------
# test_train_pointwise_cpu.py checks these numbers against the source text.
CAPS = {
    "loss": (1024, 256),               # quads of pixels, fill_loss_params
    "recurrent_fill": (4096, 256),     # float4 of the scatter buffer, isrRecurrentInputBackward
    "recurrent_post": (4096, 256),     # high-resolution pixels, isrRecurrentInputBackward
    "upsample_forward": (8192, 256),   # output quads (pairs for an odd width), isrUpsample2xForward's generic form
    "upsample_backward": (16384, 256), # input pixels, isrUpsample2xBackward's generic form
    "recon_fill": (4096, 256),         # floats of the input gradient, isrReconResidualBackward
    "act_backward": (2048, 1024),      # elements (256 threads x 4), isrActBackward
    "phase_gradient": (16384, 256),    # low-resolution pixels, isrConvTransposePhaseGradient
    "adam": (4096, 256),               # parameters, isrAdamFlatStep
}


def crosses_cap(name, items):
    """Whether a launch over ``items`` work items makes some workgroup of the capped grid go round its stride loop a second time."""
    blocks, per_block = CAPS[name]
    return items > blocks * per_block


def record_error(case, kind, error, own, bar):
    """One row of profiles/train_pointwise_errors.md appended to the file ISR_TRAIN_POINTWISE_REPORT names, if it names one."""
    path = os.environ.get("ISR_TRAIN_POINTWISE_REPORT")
    if path:
        with open(path, "a") as f:
            f.write("| %s | %s | %.2e | %.2e | %.2e |\n" % (case, kind, error, own, bar))


def recorder(prefix=""):
    return lambda label, kind, err, own, bar: record_error(prefix + label, kind, err, own, bar)


def no_border(n, h, w):
    return torch.zeros(n, h, w, dtype=torch.bool)


def edge_sets(n, h, w):
    """First and last rows and columns and the rest of [n, *, h, w] tensors (a corner pixel is in two sets)."""
    sets = {}
    for name, index in (("first row", (slice(None), 0)), ("last row", (slice(None), h - 1)),
                        ("first column", (slice(None), slice(None), 0)), ("last column", (slice(None), slice(None), w - 1))):
        m = torch.zeros(n, h, w, dtype=torch.bool)
        m[index] = True
        sets[name] = m
    union = torch.zeros(n, h, w, dtype=torch.bool)
    for m in sets.values():
        union |= m
    sets["rest"] = ~union
    return sets


# =====================================================================================================================================
# Loss: LossNetUnshaded's module path (fused = False)
# =====================================================================================================================================
RECIPE = "l1:mask:1,l1:ao:1,l1:normal:10,l1:depth:10,temp-l2:color:0.1"
EVERYTHING = ("mse:mask:0.3,mse:normal:2,mse:ao:0.7,mse:depth:1.5,mse:color:0.9,l1:mask:1,l1:normal:3,l1:ao:0.4,l1:depth:2,"
              "l1:color:0.6,temp-l2:mask:0.2,temp-l2:normal:0.8,temp-l2:ao:0.5,temp-l2:depth:1.1,temp-l2:color:0.1")
CONFIGURATIONS = {"everything": EVERYTHING, "recipe": RECIPE}
LOSS_SHAPES = [(2, 16, 16, 2), (3, 12, 20, 0), (1, 8, 8, 3)]                # (N, H, W, pad)
LOSS_CAP_SHAPE = (2, 736, 736, 4)
AO_VARIANTS = [(ao, inverse) for ao in (0.0, 0.35, 1.0) for inverse in (False, True)]
PREV_MODES = ("gradient", "no gradient", "absent")
UPSTREAM = 1.7                                                               # an upstream factor other than 1
AMBIENT, DIFFUSE = float(np.float32(0.1)), float(np.float32(0.9))            # the shader's constants as fp32 holds them


def without_temporal(losses):
    return ",".join(e for e in losses.split(",") if not e.startswith("temp-l2"))


def loss_criterion(device, losses, ao, inverse_ao, high_res, pad, fused):
    from isosurfacesuperresolution_amd import losses as L
    opt = argparse.Namespace(upsample='bilinear', losses=losses, lossAO=ao, lossAmbient=0.1, lossDiffuse=0.9, lossSpecular=0.0)
    crit = L.LossNetUnshaded(device, 5, 6, high_res, pad, opt).to(device)
    crit.shading.inverse_ao = inverse_ao
    crit.fused = fused
    return crit


def loss_module_path(gt, pred, prev, prev_mode, losses, ao, inverse_ao, pad, dtype, device="cpu"):
    """``LossNetUnshaded.forward`` with ``fused = False`` in ``dtype`` -> ({(kind, target): value}, total, d / d pred, d / d prev or None)
    of ``UPSTREAM`` x total, floats and fp64 CPU tensors.  Without ``prev`` the temp-l2 terms are left out of the configuration (the
    module path cannot run them, the kernel skips them)."""
    absent = prev_mode == "absent"
    crit = loss_criterion(device, without_temporal(losses) if absent else losses, ao, inverse_ao, gt.shape[2], pad, fused=False)
    crit.lazy_values = True
    p = pred.to(device=device, dtype=dtype).clone().requires_grad_(True)
    v = None if absent else prev.to(device=device, dtype=dtype).clone().requires_grad_(prev_mode == "gradient")
    total, values = crit(gt.to(device=device, dtype=dtype), p, None, None, v)
    (total * UPSTREAM).backward()
    gprev = v.grad.double().cpu() if prev_mode == "gradient" and v.grad is not None else None
    return {k: float(x) for k, x in values.items()}, float(total.detach()), p.grad.double().cpu(), gprev


def field_differences(pred, gt, ao_strength, inverse_ao, colour_only=False):
    """[n, 7, h, w] fp64: ``pred - gt`` of the fields the loss compares -- mask, gated normal xyz, gated ao, gated depth, colour (one
    channel: white material, the three are equal; nine with them) -- for the loss shader of the tests.  ``colour_only``: the last
    channel alone (the only one the AO variant changes)."""
    gate = (gt.double()[:, 0:1] * 0.5 + 0.5).clamp(0, 1)

    def fields(x):
        x = x.double()
        nrm = x[:, 1:4]
        a = 1.0 - x[:, 5:6] if inverse_ao else x[:, 5:6]
        aof = ao_strength * a.clamp(0, 1) + (1.0 - ao_strength)
        colour = ((x[:, 0:1] * 0.5 + 0.5).clamp(0, 1) * ((AMBIENT + DIFFUSE * nrm[:, 2:3].abs()) * aof)).clamp(0, 1)
        if colour_only:
            return colour
        nh = nrm / nrm.norm(dim=1, keepdim=True).clamp_min(1e-7)
        return torch.cat([x[:, 0:1], nh * gate, x[:, 5:6] * gate, x[:, 4:5] * gate, colour], dim=1)

    return fields(pred) - fields(gt)


def _close_to_l1_kink(pred, gt):
    """[n, h, w]: a field difference that is not exactly 0 lies within CLEAR of 0, under some AO variant."""
    near = torch.zeros(pred.shape[0], pred.shape[2], pred.shape[3], dtype=torch.bool)
    for k, (ao, inverse) in enumerate(AO_VARIANTS):
        d = field_differences(pred, gt, ao, inverse, colour_only=k > 0)
        near |= ((d != 0) & (d.abs() < CLEAR)).any(dim=1)
    return near


def l1_clearance(pred, gt, where, ao_strength, inverse_ao):
    """Smallest |field difference| that is not exactly 0 over the pixels ``where`` [n, h, w]."""
    d = field_differences(pred, gt, ao_strength, inverse_ao).permute(0, 2, 3, 1)[where]
    d = d[d != 0].abs()
    return float(d.min()) if d.numel() else float("inf")


def loss_operands(n, h, w, pad, seed=7):
    """(gt, pred, prev) fp32 [n, 6, h, w] on the CPU and {kind: [n, h, w] mask} of the planted pixels.  ``pred`` and ``prev`` carry
    ``discr_input_common.plant``'s seven kinks at the same pixels; three pixels more: ``pred == gt`` in all six channels (mask 0.5, so
    the gate is open: every l1 gradient is exactly 0 there and only the temp-l2 terms reach it) and ``gt`` mask = +1 / -1 (a gate of
    exactly 1 / exactly 0).  Where the interior is 2 x 2 the three share pixels with the seven."""
    gt, pred, prev = field6(seed, n, h, w), field6(seed + 1, n, h, w), field6(seed + 2, n, h, w)
    inside = torch.zeros(n, h, w, dtype=torch.bool)
    inside[:, pad:h - pad, pad:w - pad] = True
    at = (_close_to_l1_kink(pred, gt) & inside).nonzero(as_tuple=True)         # (image, row, column) of the pixels still to move
    for attempt in range(40):
        if not at[0].numel():
            break
        drawn = field6(seed + 100 + attempt, n, h, w)[at[0], :, at[1], at[2]]   # [K, 6]
        pred[at[0], :, at[1], at[2]] = drawn
        as_image = lambda t: t.t().reshape(1, 6, 1, -1)
        still = _close_to_l1_kink(as_image(drawn), as_image(gt[at[0], :, at[1], at[2]])).view(-1)
        at = tuple(i[still] for i in at)
    else:
        raise AssertionError("the l1 kinks could not be cleared")
    planted = plant(pred, pad)
    plant(prev, pad)
    taken = torch.zeros(h, w, dtype=torch.bool)
    for m in planted.values():
        taken |= m[0]
    free = (inside[0] & ~taken).nonzero().tolist()                     # interior pixels of image 0 in row-major order
    if len(free) >= 3:
        same, plus, minus = free[len(free) // 4], free[len(free) // 2], free[(3 * len(free)) // 4]
    else:
        pixels = inside[0].nonzero().tolist()
        same, plus, minus = pixels[3], pixels[2], pixels[0]            # beside |normal| = 5e-8, normal = 0 and the first group
    pred[0, 0, same[0], same[1]] = 0.5
    gt[0, :, same[0], same[1]] = pred[0, :, same[0], same[1]]
    gt[0, 0, plus[0], plus[1]] = 1.0
    gt[0, 0, minus[0], minus[1]] = -1.0
    for kind, (yy, xx) in (("pred=gt", same), ("gt mask=+1", plus), ("gt mask=-1", minus)):
        planted[kind] = torch.zeros(n, h, w, dtype=torch.bool)
        planted[kind][0, yy, xx] = True
    return (gt, pred, prev), planted


def colour_one_plant():
    """The optional plant 'pre-clamp colour exactly 1' (mask 1, normal (0, 0, 1), AO argument 1): (fp32 value, fp64 value) of the
    pre-clamp colour as the module path forms it, ambient + diffuse |n_z| with the shader's fp32 constants."""
    a32, d32 = torch.tensor(0.1, dtype=torch.float32), torch.tensor(0.9, dtype=torch.float32)
    return float(a32 + d32 * 1.0), float(a32.double() + d32.double() * 1.0)


# =====================================================================================================================================
# Recurrent input: clamp / normalize / warp_upscale(.., 4, special_mask=True) / flatten_high / cat
# =====================================================================================================================================
RECURRENT_SHAPES = [(2, 5, 66), (1, 3, 17)]                                # (b, h, w)
RECURRENT_CAP_SHAPE = (1, 128, 520)
FLOW_REGIMES = ("zero", "near", "far")
SC_TH, SC_TW, SC_R = 16, 64, 4                                             # the scatter's tile and LDS halo (checked against the source)
RAW_KINDS = {"mask=+1": {0: 1.0}, "mask=-1": {0: -1.0}, "depth=0": {4: 0.0}, "depth=1": {4: 1.0}, "ao=0": {5: 0.0}, "ao=1": {5: 1.0},
             "normal=0": {1: 0.0, 2: 0.0, 3: 0.0}, "|normal|=5e-8": {1: 0.0, 2: 0.0, 3: TINY}}


def raw6(seed, b, H, W):
    """[b, 6, H, W] fp32 raw prediction: mask in [-1.5, 1.5], normal in [-1, 1]^3, depth and ao in [-0.5, 1.5] (every clamp is taken on
    both sides), each clamp bound CLEAR away and |normal| >= 0.05."""
    rs = np.random.RandomState(seed)
    x = np.empty((b, 6, H, W), dtype=np.float32)
    x[:, 0] = rs.uniform(-1.5, 1.5, (b, H, W))
    x[:, 1:4] = rs.uniform(-1.0, 1.0, (b, 3, H, W))
    x[:, 4:6] = rs.uniform(-0.5, 1.5, (b, 2, H, W))
    m, nx = x[:, 0], x[:, 1]
    m[np.abs(np.abs(m) - 1.0) < 2 * CLEAR] = 0.25
    for c in (4, 5):
        v = x[:, c]
        v[(np.abs(v) < 2 * CLEAR) | (np.abs(v - 1.0) < 2 * CLEAR)] = 0.5
    nx[np.sqrt((x[:, 1:4] ** 2).sum(axis=1)) < 0.05] = 0.5
    return torch.from_numpy(x)


def plant_raw(x):
    """Writes RAW_KINDS' exact values into pixels of image 0 spread over the image (in place) -> {kind: [b, H, W] mask}."""
    b, _, H, W = x.shape
    masks = {}
    for k, (kind, values) in enumerate(RAW_KINDS.items()):
        yy, xx = divmod(((k + 1) * H * W) // (len(RAW_KINDS) + 1) + 3 * k, W)
        for channel, value in values.items():
            x[0, channel, yy, xx] = value
        masks[kind] = torch.zeros(b, H, W, dtype=torch.bool)
        masks[kind][0, yy, xx] = True
    return masks


def raw_clearance(x, where):
    """Smallest distance of a raw prediction's kink quantity from its kink over the pixels ``where`` [b, H, W], in fp64."""
    v = x.double().permute(0, 2, 3, 1)[where]
    if v.numel() == 0:
        return float("inf")
    distances = [(v[:, 0].abs() - 1).abs(), v[:, 4].abs(), (v[:, 4] - 1).abs(), v[:, 5].abs(), (v[:, 5] - 1).abs(),
                 (v[:, 1:4].norm(dim=1) - 1e-7).abs()]
    return min(float(d.min()) for d in distances)


def make_flow(regime, b, h, w, seed):
    """[b, 3, 2, h, w] fp32 clip of flows (the tests take frame 2: a view with a batch stride).  A flow f moves the sample by
    f_x (W - 1) and f_y (H - 1) high-resolution pixels.  'zero': none; 'near': at most 3 pixels either way (every tap stays inside the
    scatter's LDS window, taps cross tile seams in X and Y); 'far': 4 to 12 pixels, and in the first rows / last rows / first columns /
    last columns 12 pixels outwards, so that samples leave the image on each of the four sides."""
    H, W = 4 * h, 4 * w
    rs = np.random.RandomState(seed)
    f = np.zeros((b, 3, 2, h, w), dtype=np.float32)
    if regime == "near":
        f[:, :, 0] = rs.uniform(-3.0, 3.0, (b, 3, h, w)) / (W - 1)
        f[:, :, 1] = rs.uniform(-3.0, 3.0, (b, 3, h, w)) / (H - 1)
    elif regime == "far":
        mag = rs.uniform(4.0, 12.0, (b, 3, 2, h, w))
        sign = np.where(rs.uniform(size=(b, 3, 2, h, w)) < 0.5, -1.0, 1.0)
        shift = mag * sign                                          # in high-resolution pixels: x sample = X - f_x (W - 1), y sample = Y + f_y (H - 1)
        shift[:, :, 0, :, 0] = 12.0; shift[:, :, 0, :, -1] = -12.0  # first columns sample to the left, last columns to the right
        shift[:, :, 1, 0, :] = -12.0; shift[:, :, 1, -1, :] = 12.0  # first rows sample above, last rows below
        f[:, :, 0] = shift[:, :, 0] / (W - 1)
        f[:, :, 1] = shift[:, :, 1] / (H - 1)
    elif regime != "zero":
        raise ValueError(regime)
    return torch.from_numpy(f)


def sample_positions(flow):
    """(sx, sy) [b, H, W] fp64: the pixel position each high-resolution pixel samples the previous frame at (warp_upscale, x4)."""
    flow = flow.double()
    b, _, h, w = flow.shape
    H, W = 4 * h, 4 * w
    scale = torch.tensor([-2.0, 2.0], dtype=torch.float64).view(1, 2, 1, 1)
    up = F.interpolate(flow * scale, scale_factor=4, mode='bilinear', align_corners=False)
    gx = torch.linspace(-1, 1, W, dtype=torch.float64).view(1, 1, W) + up[:, 0]
    gy = torch.linspace(-1, 1, H, dtype=torch.float64).view(1, H, 1) + up[:, 1]
    return (gx + 1.0) * (0.5 * (W - 1)), (gy + 1.0) * (0.5 * (H - 1))


def previous_output(raw):
    from isosurfacesuperresolution_amd.utils import ScreenSpaceShading
    return torch.cat([torch.clamp(raw[:, 0:1], -1, +1), ScreenSpaceShading.normalize(raw[:, 1:4], dim=1),
                      torch.clamp(raw[:, 4:5], 0, +1), torch.clamp(raw[:, 5:6], 0, +1)], dim=1)


def recurrent_definition(raw, inp, flow, dtype, device="cpu", g_netin=None, g_warped=None):
    """The module path of train.clip_loss in ``dtype`` -> (net_input, warped, d / d raw or None) as fp64 CPU tensors; the gradient is
    that of sum(net_input g_netin) + sum(warped g_warped) over the upstreams that are given."""
    from isosurfacesuperresolution_amd.models import VideoTools
    to = lambda t: t.to(device=device, dtype=dtype)
    r = to(raw).clone().requires_grad_(g_netin is not None or g_warped is not None)
    warped = VideoTools.warp_upscale(previous_output(r), to(flow), 4, special_mask=True)
    netin = torch.cat((to(inp), VideoTools.flatten_high(warped, 4)), dim=1)
    grad = None
    if r.requires_grad:
        total = 0.0
        if g_netin is not None:
            total = total + (netin * to(g_netin)).sum()
        if g_warped is not None:
            total = total + (warped * to(g_warped)).sum()
        total.backward()
        grad = r.grad.double().cpu()
    return netin.detach().double().cpu(), warped.detach().double().cpu(), grad


def recurrent_sets(planted, b, H, W):
    """The backward's pixel sets [b, H, W]: within SC_R of a vertical / horizontal seam of the scatter's tiles, the image's outer ring,
    the planted raw kinks, the rest (a pixel may be in several of the first three; ``rest`` is what none of them holds)."""
    X = torch.arange(W).view(1, 1, W).expand(b, H, W)
    Y = torch.arange(H).view(1, H, 1).expand(b, H, W)
    any_planted = torch.zeros(b, H, W, dtype=torch.bool)
    for m in planted.values():
        any_planted |= m
    seam_x = ((X % SC_TW < SC_R) | (X % SC_TW >= SC_TW - SC_R)) & (X >= SC_R) & ~any_planted     # (the first tile's left edge is the ring's)
    seam_y = ((Y % SC_TH < SC_R) | (Y % SC_TH >= SC_TH - SC_R)) & (Y >= SC_R) & ~any_planted
    ring = ((X == 0) | (X == W - 1) | (Y == 0) | (Y == H - 1)) & ~any_planted
    sets = {"seam in X": seam_x, "seam in Y": seam_y, "outer ring": ring}
    sets.update(planted)
    sets["rest"] = ~(seam_x | seam_y | ring | any_planted)
    return sets


def frames(clip_in, clip_flow):
    """The frame views the tests hand to the kernels: [b, 5, h, w] and [b, 2, h, w] with the clip's batch strides."""
    return clip_in[:, 1], clip_flow[:, 2]


def recurrent_operands(b, h, w, regime, seed=3):
    """(raw [b, 6, 4h, 4w], input clip [b, 3, 5, h, w], flow clip [b, 3, 2, h, w], g_netin, g_warped) fp32 on the CPU and the planted
    kinds; ``frames`` takes the views of one frame."""
    H, W = 4 * h, 4 * w
    raw = raw6(seed, b, H, W)
    planted = plant_raw(raw)
    rs = np.random.RandomState(seed + 1)
    clip_in = torch.from_numpy(rs.uniform(-1.0, 1.0, (b, 3, 5, h, w)).astype(np.float32))
    flow = make_flow(regime, b, h, w, seed + 2)
    gn = torch.from_numpy(rs.uniform(-1.0, 1.0, (b, 101, h, w)).astype(np.float32))
    gw = torch.from_numpy(rs.uniform(-1.0, 1.0, (b, 6, H, W)).astype(np.float32))
    return (raw, clip_in, flow, gn, gw), planted


# the normal channels of `warped` against the fp32 module path: the kernel forms |n|^2 as x x + y y + z z with whatever contraction the
# compiler chose and the framework with its own reduction: two roundings of the sum may differ (2 U relative), the square root keeps
# half of that and adds its own rounding, the quotient one more: a tap's normal component (|.| <= 1) differs by at most 3 U.  The
# blend is a convex combination of four taps (the same weights, bit for bit): 3 U survive, and each of its four products and three
# sums may round the other way once the taps differ (<= U each at magnitudes <= 1): 10 U in all.
WARPED_NORMAL_BAR = 10 * U


# =====================================================================================================================================
# x2 upsampling, residual reconstruction
# =====================================================================================================================================
UPSAMPLE_SHAPES = [(1, 1, 1, 4), (2, 3, 2, 8), (1, 2, 7, 12), (2, 3, 5, 6), (2, 3, 5, 7), (1, 2, 4, 1)]
UPSAMPLE_CAP_FORWARD, UPSAMPLE_CAP_BACKWARD = (4, 1, 512, 1030), (8, 1, 512, 1030)
RECON_SHAPES = [(1, 6, 5, 5, 3, 65), (2, 6, 8, 6, 5, 12), (1, 4, 7, 2, 1, 1)]        # (n, cout, cin, k, h, w)
RECON_CAP_SHAPE = (1, 6, 101, 5, 104, 104)


def uniform(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed).uniform(-1.0, 1.0, shape).astype(np.float32))


def upsample_definition(x, gy, dtype, device="cpu"):
    """``F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False)`` and its gradient for the upstream ``gy``, fp64 CPU."""
    xx = x.to(device=device, dtype=dtype).clone().requires_grad_(True)
    y = F.interpolate(xx, scale_factor=2, mode='bilinear', align_corners=False)
    y.backward(gy.to(device=device, dtype=dtype))
    return y.detach().double().cpu(), xx.grad.double().cpu()


def recon_definition(y, x, k, g, dtype, device="cpu"):
    """enhancenet's residual reconstruction: cat(y[:, :k] + bilinear_x4(x[:, :k]), y[:, k:]) -> (out, d / d y, d / d x), fp64 CPU."""
    yy = y.to(device=device, dtype=dtype).clone().requires_grad_(True)
    xx = x.to(device=device, dtype=dtype).clone().requires_grad_(True)
    up = F.interpolate(xx[:, :k], scale_factor=4, mode='bilinear', align_corners=False)
    out = torch.cat([yy[:, :k] + up, yy[:, k:]], dim=1)
    out.backward(g.to(device=device, dtype=dtype))
    return out.detach().double().cpu(), yy.grad.double().cpu(), xx.grad.double().cpu()


# =====================================================================================================================================
# Activation backward and the phase-major gradient, index by index
# =====================================================================================================================================
ACT_COUNTS = [1, 2, 3, 5, 1027]
ACT_CAP_COUNT = 2098355
PHASE_CAP_SHAPE = (1, 64, 260, 256)                                        # (N, C, h, w) of the low-resolution planes
ACTS = ("none", "relu", "leaky")
SLOPE = 0.2


def act_backward_rule(gy, y, act, slope):
    """gz[i] = gy[i] where there is no activation or y[i] > 0, gy[i] * slope elsewhere (slope 0 for 'relu'): y == 0 and -0.0 sit on the
    slope side.  In the type of ``gy``."""
    gz = gy.clone()
    if act == "none":
        return gz
    s = 0.0 if act == "relu" else slope
    flat_g, flat_y, flat_z = gy.reshape(-1), y.reshape(-1), gz.view(-1)
    closed = torch.nonzero(~(flat_y > 0)).view(-1)
    flat_z[closed] = flat_g[closed] * s
    return gz


def phase_gradient_rule(gy, y, act, slope):
    """G[n, 4 c + 2 a + b, i, j] = gz[n, c, 2 i + a, 2 j + b] of ``act_backward_rule``'s gz."""
    gz = act_backward_rule(gy, y, act, slope)
    n, c, hh, ww = gz.shape
    out = torch.empty(n, 4 * c, hh // 2, ww // 2, dtype=gz.dtype)
    for a in (0, 1):
        for b in (0, 1):
            out[:, 2 * a + b::4] = gz[:, :, a::2, b::2]
    return out


def act_operands(seed, count):
    """(gy, y) fp32 [count]: y with exact +0.0 and -0.0 among its values (every seventh and every eleventh element)."""
    rs = np.random.RandomState(seed)
    gy = torch.from_numpy(rs.uniform(-1.0, 1.0, count).astype(np.float32))
    y = torch.from_numpy(rs.uniform(-1.0, 1.0, count).astype(np.float32))
    y[::7] = 0.0
    y[3::11] = -0.0
    return gy, y


# =====================================================================================================================================
# Adam (torch.optim.Adam, no weight decay, no amsgrad)
# =====================================================================================================================================
ADAM_SIZES = [100003, 1049353]
ADAM_LRS = [1e-3, 7e-4, 2e-3, 5e-4, 1.5e-3]
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
# floors of the Adam bars, in unit roundoffs of the quantity, from the kernel's operation count over the five steps of the tests
# (gradients keep their sign per element, so neither moment cancels):
#  exp_avg: subtract, multiply, add per step = 3 roundings, 15 over five steps (an upper bound: the older ones are damped by beta1), and
#    the rounding of fp32(1 - beta1): 16 U
#  exp_avg_sq: four roundings per step (v beta2, (1 - beta2) g, . g, the sum), 20 over five steps, and the roundings of fp32(beta2) and
#    fp32(1 - beta2): 22 U
#  update / lr = q = (m / (sqrt(v) / bc2s + eps)) / bc1, |q| about 1: exp_avg's 16 U and half of exp_avg_sq's 22 U, then sqrt, divide, add,
#    divide, multiply and the rounded step_size and bc2s = 7 more: 34 U of the step's largest |q| (of order 1: between 0.5 and 8 for these
#    operands).  The update is read off the fp32 parameters as p_new - p_old, so the test adds the parameters' own rounding,
#    U max |p| / lr (the operands keep |p| small for that reason).
ADAM_FLOOR_M, ADAM_FLOOR_V, ADAM_FLOOR_UPDATE = 16 * U, 22 * U, 34 * U


def adam_signs(seed, n):
    return np.where(np.random.RandomState(seed + 7).uniform(size=n) < 0.5, -1.0, 1.0)


def adam_gradients(seed, n, steps):
    """[steps][n] fp32 gradients: magnitudes 10^U(-8, 3) per element and step, one sign per element for all steps; the first 128
    elements are 0 at every step, one element in ten is 0 at any one step."""
    rs = np.random.RandomState(seed)
    sign = adam_signs(seed, n)
    out = []
    for _ in range(steps):
        g = sign * 10.0 ** rs.uniform(-8.0, 3.0, n)
        g[rs.uniform(size=n) < 0.1] = 0.0
        g[:128] = 0.0
        out.append(torch.from_numpy(g.astype(np.float32)))
    return out


def adam_state(seed, n, warm):
    """(params, exp_avg, exp_avg_sq) fp32, |params| <= 1e-3: zero moments for a fresh optimizer, or -- ``warm`` -- moments such as a thousand
    steps leave behind (exp_avg with the sign of the element's gradients, exp_avg_sq above its square), zeros in the first 128 elements."""
    rs = np.random.RandomState(seed + 1000)
    p = torch.from_numpy((rs.uniform(-1.0, 1.0, n) * 1e-3).astype(np.float32))
    if not warm:
        return p, torch.zeros(n), torch.zeros(n)
    m = adam_signs(seed, n) * rs.uniform(0.1, 1.0, n) * 10.0 ** rs.uniform(-6.0, 1.0, n)
    v = m * m * rs.uniform(1.0, 50.0, n)
    m[:128] = 0.0
    v[:128] = 0.0
    return p, torch.from_numpy(m.astype(np.float32)), torch.from_numpy(v.astype(np.float32))


def adam_step64(p, g, m, v, t, lr):
    """Step number ``t`` (1-based) of torch.optim.Adam on float64 tensors, in place; Python-double bias corrections."""
    m.lerp_(g, 1.0 - BETA1)
    v.mul_(BETA2).addcmul_(g, g, value=1.0 - BETA2)
    bc1, bc2 = 1.0 - BETA1 ** t, 1.0 - BETA2 ** t
    denom = (v.sqrt() / bc2 ** 0.5).add_(EPS)
    p.addcdiv_(m, denom, value=-lr / bc1)


def adam_trajectory(step_fn, p, m, v, grads, lrs):
    """Runs ``step_fn(p, g, m, v, k, lr)`` over the steps -> ([update per step], m, v) as fp64 CPU tensors."""
    updates = []
    for k, (g, lr) in enumerate(zip(grads, lrs)):
        before = p.detach().double().cpu().clone()
        step_fn(p, g, m, v, k, lr)
        updates.append(p.detach().double().cpu() - before)
    return updates, m.detach().double().cpu(), v.detach().double().cpu()


def adam_reference(dtype, p0, m0, v0, grads, lrs, first_step):
    """float64: ``adam_step64``; float32: torch.optim.Adam itself with its state set to (first_step, m0, v0)."""
    p, m, v = (t.to(dtype).clone() for t in (p0, m0, v0))
    if dtype == torch.float64:
        return adam_trajectory(lambda p, g, m, v, k, lr: adam_step64(p, g.double(), m, v, first_step + k + 1, lr), p, m, v, grads, lrs)
    p.requires_grad_(True)
    optim = torch.optim.Adam([p], lr=lrs[0], betas=(BETA1, BETA2), eps=EPS)
    optim.state[p] = {"step": torch.tensor(float(first_step)), "exp_avg": m, "exp_avg_sq": v}

    def step(p, g, m, v, k, lr):
        optim.param_groups[0]["lr"] = lr
        p.grad = g.clone()
        optim.step()

    return adam_trajectory(step, p, m, v, grads, lrs)


def relative_error(got, ref):
    """Largest |got - ref| / |ref| over the elements with ref != 0; where ref == 0, got must be exactly 0."""
    zero = ref == 0
    assert not got[zero].any(), "a value that is exactly 0 in the reference is not 0"
    if zero.all():
        return 0.0
    return float(((got[~zero] - ref[~zero]).abs() / ref[~zero].abs()).max())
