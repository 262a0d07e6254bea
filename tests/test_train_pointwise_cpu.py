"""CPU: what tests/test_train_pointwise_gpu.py relies on, asserted on the operands and definitions themselves (train_pointwise_common) --
the planted pixels sit exactly on their kinks in fp32 and fp64, every other pixel is CLEAR of every kink on every operand set the GPU
file uses, the index-by-index activation and phase rules equal autograd in fp64, the CPU branches of ``ops`` and of the loss equal the
definitions, the caps the cap cases are computed from are the source's, and each cap case crosses its cap.  The fp32-to-fp64
distances that serve as bars on the device are printed (``pytest -s``)."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import train_pointwise_common as P
from discr_input_common import CLEAR, TINY, kink_clearance, pixel_sets

SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "isosurfacesuperresolution_amd", "csrc", "sr_train.hip")


def _pixel(x, mask):
    return x.permute(0, 2, 3, 1)[mask][0]


@pytest.mark.parametrize("shape", P.LOSS_SHAPES + [(1, 64, 64, 4)], ids=lambda s: "%dx%dx%d_pad%d" % s)
def test_loss_operands_planted_pixels_and_clearance(shape):
    n, h, w, pad = shape
    (gt, pred, prev), planted = P.loss_operands(n, h, w, pad)
    assert set(planted) == {"mask=+1", "mask=-1", "ao=0", "ao=1", "normal=0", "|normal|=5e-8", "n_z=0", "pred=gt", "gt mask=+1", "gt mask=-1"}
    sets, border = pixel_sets(planted, n, h, w, pad)
    for m in planted.values():
        assert int(m.sum()) == 1 and not bool((m & border).any())
    for x in (pred, prev):
        assert _pixel(x, planted["mask=+1"])[0] == 1.0 and _pixel(x, planted["mask=-1"])[0] == -1.0
        assert _pixel(x, planted["ao=0"])[5] == 0.0 and _pixel(x, planted["ao=1"])[5] == 1.0
        assert not _pixel(x, planted["normal=0"])[1:4].any() and _pixel(x, planted["n_z=0"])[3] == 0.0
        for dtype in (torch.float32, torch.float64):
            length = _pixel(x, planted["|normal|=5e-8"])[1:4].to(dtype).norm()
            assert 0 < float(length) < 1e-7 and abs(float(length) - 5e-8) < 1e-14
    same = planted["pred=gt"]
    assert torch.equal(_pixel(pred, same), _pixel(gt, same)) and _pixel(gt, same)[0] == 0.5
    assert _pixel(gt, planted["gt mask=+1"])[0] == 1.0 and _pixel(gt, planted["gt mask=-1"])[0] == -1.0
    for dtype in (torch.float32, torch.float64):                     # the gates are exactly 1 and exactly 0, the differences exactly 0
        gate = lambda kind: float((_pixel(gt, planted[kind])[0].to(dtype) * 0.5 + 0.5).clamp(0, 1))
        assert gate("gt mask=+1") == 1.0 and gate("gt mask=-1") == 0.0
    for ao, inverse in P.AO_VARIANTS:
        assert not P.field_differences(pred, gt, ao, inverse).permute(0, 2, 3, 1)[same].any()
        # every other interior pixel: the shader's kinks (pred and prev are shaded from the normal as it arrives) and l1's
        for x in (pred, prev):
            assert kink_clearance(x, sets["rest"], True, ao, inverse) >= CLEAR
        assert P.l1_clearance(pred, gt, sets["rest"], ao, inverse) >= CLEAR
    # moved, not excluded: the sets hold every pixel
    union = border.clone()
    for m in sets.values():
        union |= m
    assert bool(union.all())


def test_the_optional_colour_one_plant_is_left_out_because_the_precisions_disagree():
    """Mask 1, normal (0, 0, 1), AO argument 1 gives a pre-clamp colour of ambient + diffuse: fp32(0.1) + fp32(0.9) rounds to exactly 1
    in fp32 and is 1 - 2.2e-8 in fp64 -- the two module paths do not land on the same side of the clamp's bound, so the plant would
    compare two different branches.  It is not planted."""
    c32, c64 = P.colour_one_plant()
    assert c32 == 1.0 and c64 < 1.0 and 1.0 - c64 < 1e-7


@pytest.mark.parametrize("shape", P.RECURRENT_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_recurrent_operands_planted_pixels_clearance_and_flows(shape):
    b, h, w = shape
    H, W = 4 * h, 4 * w
    for regime in P.FLOW_REGIMES:
        (raw, clip_in, clip_flow, gn, gw), planted = P.recurrent_operands(b, h, w, regime)
        inp, flow = P.frames(clip_in, clip_flow)
        assert set(planted) == set(P.RAW_KINDS)
        assert not inp.is_contiguous() or b == 1
        at = lambda kind: _pixel(raw, planted[kind])
        assert at("mask=+1")[0] == 1.0 and at("mask=-1")[0] == -1.0 and at("depth=0")[4] == 0.0 and at("depth=1")[4] == 1.0
        assert at("ao=0")[5] == 0.0 and at("ao=1")[5] == 1.0 and not at("normal=0")[1:4].any()
        for dtype in (torch.float32, torch.float64):
            length = at("|normal|=5e-8")[1:4].to(dtype).norm()
            assert 0 < float(length) < 1e-7 and abs(float(length) - 5e-8) < 1e-14
        sets = P.recurrent_sets(planted, b, H, W)
        union = torch.zeros(b, H, W, dtype=torch.bool)
        for m in sets.values():
            union |= m
        assert bool(union.all())
        unplanted = union.clone()
        for m in planted.values():
            assert int(m.sum()) == 1
            unplanted &= ~m
        assert P.raw_clearance(raw, unplanted) >= CLEAR
        # the regimes do what their names say, in high-resolution pixels
        sx, sy = P.sample_positions(flow)
        X = torch.arange(W, dtype=torch.float64).view(1, 1, W)
        Y = torch.arange(H, dtype=torch.float64).view(1, H, 1)
        dx, dy = (sx - X).abs(), (sy - Y).abs()
        if regime == "zero":
            assert float(dx.max()) < 1e-9 and float(dy.max()) < 1e-9
        elif regime == "near":
            assert float(dx.max()) <= 3.0 + 1e-5 and float(dy.max()) <= 3.0 + 1e-5 and float(dx.max()) > 2.0
        else:
            assert float(torch.maximum(dx, dy).max()) <= 12.0 + 1e-5 and float(dx.max()) > P.SC_R
            assert bool((sx < -1).any()) and bool((sx > W).any()) and bool((sy < -1).any()) and bool((sy > H).any())
    if shape == (2, 5, 66):
        assert (W + P.SC_TW - 1) // P.SC_TW == 5 and W % P.SC_TW == 8 and (H + P.SC_TH - 1) // P.SC_TH == 2 and H % P.SC_TH == 4
        assert 4 * w - 256 == 8                                          # live threads of the forward's second workgroup


@pytest.mark.parametrize("act", P.ACTS)
def test_index_by_index_rules_equal_autograd_in_fp64(act):
    gy, y0 = P.act_operands(5, 2 * 3 * 6 * 10)
    gy, z = gy.double().view(2, 3, 6, 10), y0.double().view(2, 3, 6, 10).clone().requires_grad_(True)
    y = {"none": lambda t: t * 1.0, "relu": torch.relu, "leaky": lambda t: F.leaky_relu(t, P.SLOPE)}[act](z)
    assert bool((y == 0).any()) or act == "none"
    (auto,) = torch.autograd.grad(y, z, gy)
    assert torch.equal(P.act_backward_rule(gy, y.detach(), act, P.SLOPE), auto)
    assert torch.equal(P.phase_gradient_rule(gy, y.detach(), act, P.SLOPE), F.pixel_unshuffle(auto, 2))
    # and ops' CPU branch of the phase gradient is the same rule in fp32
    from isosurfacesuperresolution_amd import ops
    g32, y32 = gy.float(), y.detach().float()
    assert torch.equal(ops.conv_transpose_phase_gradient(g32, None if act == "none" else y32, act, P.SLOPE), P.phase_gradient_rule(g32, y32, act, P.SLOPE))


def test_zero_and_negative_zero_sit_on_the_slope_side():
    gy = torch.tensor([2.0, 2.0, 2.0, 2.0])
    y = torch.tensor([0.0, -0.0, 1e-30, -1.0])
    assert P.act_backward_rule(gy, y, "relu", P.SLOPE).tolist() == [0.0, 0.0, 2.0, 0.0]
    assert torch.equal(P.act_backward_rule(gy, y, "leaky", 0.5), torch.tensor([1.0, 1.0, 2.0, 1.0]))
    assert torch.equal(P.act_backward_rule(gy, y, "none", 0.5), gy)


@pytest.mark.parametrize("shape", P.UPSAMPLE_SHAPES, ids=str)
def test_cpu_branch_of_the_upsampling_equals_the_definition(shape):
    from isosurfacesuperresolution_amd import ops
    x, gy = P.uniform(1, *shape), P.uniform(2, shape[0], shape[1], 2 * shape[2], 2 * shape[3])
    xx = x.clone().requires_grad_(True)
    y = ops.bilinear_upsample2x(xx)
    y.backward(gy)
    y32, g32 = P.upsample_definition(x, gy, torch.float32)
    y64, g64 = P.upsample_definition(x, gy, torch.float64)
    assert torch.equal(y.detach().double(), y32) and torch.equal(xx.grad.double(), g32)
    print("upsample %s: fp32-vs-fp64 values %.3e gradient %.3e" % (shape, float((y32 - y64).abs().max()), float((g32 - g64).abs().max())))
    assert float((y32 - y64).abs().max()) <= 4 * P.U and float((g32 - g64).abs().max()) <= 64 * P.U


@pytest.mark.parametrize("prev_mode", P.PREV_MODES)
def test_cpu_branch_of_the_loss_equals_the_definition(prev_mode):
    """A criterion with ``fused = True`` given CPU tensors runs the module path: the same bits as the definition in fp32; and the
    definition's fp32-to-fp64 distances, printed."""
    n, h, w, pad = P.LOSS_SHAPES[0]
    (gt, pred, prev), planted = P.loss_operands(n, h, w, pad)
    sets, border = pixel_sets(planted, n, h, w, pad)
    losses = P.EVERYTHING
    crit = P.loss_criterion("cpu", P.without_temporal(losses) if prev_mode == "absent" else losses, 0.35, True, h, pad, fused=True)
    p = pred.clone().requires_grad_(True)
    v = None if prev_mode == "absent" else prev.clone().requires_grad_(prev_mode == "gradient")
    total, values = crit(gt, p, None, None, v)
    (total * P.UPSTREAM).backward()
    v32, t32, gp32, gv32 = P.loss_module_path(gt, pred, prev, prev_mode, losses, 0.35, True, pad, torch.float32)
    v64, t64, gp64, gv64 = P.loss_module_path(gt, pred, prev, prev_mode, losses, 0.35, True, pad, torch.float64)
    assert float(total.detach()) == t32 and {k: float(x) for k, x in values.items()} == v32
    assert torch.equal(p.grad.double(), gp32)
    assert (gv32 is None) == (prev_mode != "gradient")
    if gv32 is not None:
        assert torch.equal(v.grad.double(), gv32)
    assert set(v64) == set(v32) and len(v64) == (10 if prev_mode == "absent" else 15)
    print("loss values, prev %s: fp32-vs-fp64 %.3e (total %.3e)" % (prev_mode, max(abs(v32[k] - v64[k]) for k in v64), abs(t32 - t64)))
    assert not P.compare("loss d/d pred, prev " + prev_mode, gp32, gp64, gp32, sets, border, True, 1e-5)       # (prints the distances)
    assert abs(t32 - t64) <= 1e-5 * abs(t64)


@pytest.mark.parametrize("shape", P.RECURRENT_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_recurrent_definition_in_both_precisions(shape):
    """The definition runs in fp32 and fp64, its border behaviour is the one the device test asserts (a sample more than a pixel outside
    the image gives mask -1 and zeros), and its fp32-to-fp64 distances are printed."""
    b, h, w = shape
    H, W = 4 * h, 4 * w
    for regime in P.FLOW_REGIMES:
        (raw, clip_in, clip_flow, gn, gw), planted = P.recurrent_operands(b, h, w, regime)
        inp, flow = P.frames(clip_in, clip_flow)
        n32, w32, g32 = P.recurrent_definition(raw, inp, flow, torch.float32, g_netin=gn, g_warped=gw)
        n64, w64, g64 = P.recurrent_definition(raw, inp, flow, torch.float64, g_netin=gn, g_warped=gw)
        assert torch.equal(n32[:, 0:5], inp.double()) and n32.shape == (b, 101, h, w) and w32.shape == (b, 6, H, W)
        sx, sy = P.sample_positions(flow)
        outside = (sx < -1.001) | (sx > W + 0.001) | (sy < -1.001) | (sy > H + 0.001)
        for ww in (w32, w64):
            far = ww.permute(0, 2, 3, 1)[outside]
            assert bool((far[:, 0] == -1.0).all()) and not far[:, 1:].any()
        assert bool(outside.any()) or regime != "far"
        print("recurrent %s %s: fp32-vs-fp64 warped %.3e d/d raw %.3e (largest %.3e)"
              % (shape, regime, float((w32 - w64).abs().max()), float((g32 - g64).abs().max()), float(g64.abs().max())))


def test_adam_cpu_branch_and_reference_distances():
    """``ops.adam_flat_step`` on CPU tensors is torch.optim.Adam's arithmetic: the same bits as the optimizer itself, for a fresh state and
    for a step counter of 1000; and the optimizer's own fp32-to-fp64 distances (what the device bars are four times of), printed."""
    from isosurfacesuperresolution_amd import ops
    n = 4099
    for first_step, warm in ((0, False), (1000, True)):
        grads = P.adam_gradients(11, n, len(P.ADAM_LRS))
        p0, m0, v0 = P.adam_state(11, n, warm)
        u32, m32, v32 = P.adam_reference(torch.float32, p0, m0, v0, grads, P.ADAM_LRS, first_step)
        u64, m64, v64 = P.adam_reference(torch.float64, p0, m0, v0, grads, P.ADAM_LRS, first_step)
        p, m, v, step = p0.clone(), m0.clone(), v0.clone(), torch.tensor([float(first_step)])
        ucpu, mcpu, vcpu = P.adam_trajectory(lambda p, g, m, v, k, lr: ops.adam_flat_step(p, g, m, v, step, lr, P.BETA1, P.BETA2, P.EPS),
                                             p, m, v, grads, P.ADAM_LRS)
        assert float(step) == first_step + len(P.ADAM_LRS)
        assert torch.equal(mcpu, m32) and torch.equal(vcpu, v32) and all(torch.equal(a, b) for a, b in zip(ucpu, u32))
        assert not m64[:128].any() and not v64[:128].any() and not any(u[:128].any() for u in u64)
        own_m, own_v = P.relative_error(m32, m64), P.relative_error(v32, v64)
        own_u = max(float(((a - r) / lr).abs().max()) for a, r, lr in zip(u32, u64, P.ADAM_LRS))
        print("adam from step %d: fp32-vs-fp64 exp_avg %.3e exp_avg_sq %.3e update / lr %.3e (floors %.3e %.3e %.3e)"
              % (first_step, own_m, own_v, own_u, P.ADAM_FLOOR_M, P.ADAM_FLOOR_V, P.ADAM_FLOOR_UPDATE))
        assert own_m <= P.ADAM_FLOOR_M and own_v <= P.ADAM_FLOOR_V          # the derivation of the floors holds for the framework's own fp32 step
        assert 0.5 <= max(float((u / lr).abs().max()) for u, lr in zip(u64, P.ADAM_LRS)) <= 8.0     # |update / lr| is of order 1


def test_caps_are_the_sources_and_each_cap_case_crosses_its_cap():
    text = open(SOURCE).read()
    count = lambda pattern: len(re.findall(pattern, text))
    assert count(r"P\.blocks = \(int\)\(blocks > 1024 \? 1024 : blocks\);") == 1 and count(r"long long blocks = \(quads \+ 255\) / 256;\n    P\.blocks") == 1
    assert count(r"if \(zb > 4096\) zb = 4096;") == 2 and count(r"if \(blocks > 4096\) blocks = 4096;") == 1
    assert count(r"if \(blocks > 8192\) blocks = 8192;") == 2 and count(r"if \(blocks > 16384\) blocks = 16384;") == 2
    assert count(r"long long blocks = \(count / 4 \+ 255\) / 256;\n    if \(blocks > 2048\) blocks = 2048;") == 1
    assert count(r"dim3\(\(unsigned\)\(blocks > 4096 \? 4096 : blocks\)\), dim3\(256\)") == 1
    assert count(r"constexpr int SC_TH = 16, SC_TW = 64, SC_R = 4;") == 1 and (P.SC_TH, P.SC_TW, P.SC_R) == (16, 64, 4)
    n, h, w, _ = P.LOSS_CAP_SHAPE
    assert n * h * (w // 4) == 270848 and P.crosses_cap("loss", n * h * (w // 4))
    assert not any(P.crosses_cap("loss", n * h * (w // 4)) for n, h, w, _ in P.LOSS_SHAPES)
    b, h, w = P.RECURRENT_CAP_SHAPE
    assert 16 * b * h * w == 1064960 and P.crosses_cap("recurrent_post", 16 * b * h * w) and P.crosses_cap("recurrent_fill", 16 * b * h * w * 6 // 4)
    n, c, h, w = P.UPSAMPLE_CAP_FORWARD
    assert w % 2 == 0 and w % 4 != 0 and P.crosses_cap("upsample_forward", n * c * 2 * h * (2 * w // 4))      # the generic <4> form
    n, c, h, w = P.UPSAMPLE_CAP_BACKWARD
    assert w % 4 != 0 and P.crosses_cap("upsample_backward", n * c * h * w)
    n, cout, cin, k, h, w = P.RECON_CAP_SHAPE
    assert P.crosses_cap("recon_fill", n * cin * h * w)
    assert P.crosses_cap("act_backward", P.ACT_CAP_COUNT) and P.ACT_CAP_COUNT % 4 == 3 and not P.crosses_cap("act_backward", max(P.ACT_COUNTS))
    n, c, h, w = P.PHASE_CAP_SHAPE
    assert P.crosses_cap("phase_gradient", n * c * h * w)
    assert [P.crosses_cap("adam", n) for n in P.ADAM_SIZES] == [False, True]


def test_entry_points_refuse_misaligned_loss_operands_in_the_source():
    """The host-side alignment checks this file's device twin tests by return code are in the source (a CPU box cannot call them with
    device pointers; a host pointer is as good for a check that launches nothing, see the device test)."""
    text = open(SOURCE).read()
    assert "if (!aligned16(gt) || !aligned16(pred) || !aligned16(prev)) return -1;" in text
    assert "!aligned16(gpred) || !aligned16(gprev)" in text
