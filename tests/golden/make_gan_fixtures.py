"""Generates tests/golden/gan_reference.npz: the reference's discriminators, the adversarial terms of its LossNetUnshaded and one
adversarial optimisation step of its trainer (mainVideoUnshaded.py:506-624, ``trainAdv_v2``).

The reference's Python modules (`losses`, `models`, `utils`) are IMPORTED from a checkout of the reference (its SuperresolutionNetwork
directory, given on the command line), unmodified, in the manner of make_rcan_fixtures.py: torch CPU, fp32, one thread, deterministic
algorithms, `F.grid_sample` forced to `align_corners=True`.  Two shims make the import and the criterion run on a current torch:
  * an empty stand-in for `torchvision` (lossbuilder.py:6 imports it; only the VGG terms use it);
  * `torch.full` defaulting to the float dtype (lossbuilder.py:241 builds its labels with an integer fill value, which current torch
    turns into int64 and `binary_cross_entropy_with_logits` then refuses).

No weights and no inputs are stored: both sides draw them from `numpy.random.RandomState` streams (tests/gan_common.py, imported here).

Conditions asserted on what is recorded:
  (1) every recorded value is within 4e-5 (the project's premise for its 1e-4 comparisons) of the same computation in fp64;
  (2) at least a quarter of the recorded logits have |logit| >= 0.5 (a loss of ln 2 whatever the convolutions compute cannot pass);
  (3) every convolution of every discriminator has at least 25 % of its pre-activations of each sign (both LeakyReLU branches run).

Cases:
  a  enhanceNetSmall at 16 x 16 (26 channels) and 32 x 32 (13), enhanceNetLarge at 16 x 16 (16) and 32 x 32 (26), N = 3: `state_dict`
     keys and shapes, logits;
  b  LossNetUnshaded at 16 x 16, padding 2, B = 2, enhanceNetLarge, losses gan_common.LOSSES_B: total, value dict, the gradients of
     `pred` and of `prev_pred_warped`, and the three returns of `train_discriminator`;
  c  one adversarial step written out below against the reference's modules: B = 2, T = 3, 4 x 4 -> 16 x 16, the reference's EnhanceNet
     (ten residual blocks: its constructor has no option for fewer), enhanceNetSmall, losses gan_common.LOSSES_C, torch.optim.SGD on
     both sides: the four returns (loss of the last discriminator step, loss of the last generator step, scores summed over
     discriminator steps and frames) and every parameter's change (samples, gan_common.sample_indices, and the largest |change| per tensor); the same step in fp64 gives `c_cpu32_vs_fp64`:
     per tensor the largest difference of the sampled changes, relative to the tensor's largest change.

Run:  python tests/golden/make_gan_fixtures.py <reference checkout>/SuperresolutionNetwork
"""
import functools
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "gan_reference.npz")
PREMISE = 4e-5
sys.path.insert(0, os.path.dirname(HERE))
import gan_common as C  # noqa: E402


def check_signs(discr, x, what):
    """Condition (3) on every convolution of `discr` for the input x."""
    seen = []
    hooks = [m.register_forward_hook(lambda m, i, o: seen.append(float((o > 0).float().mean()))) for m in discr.modules()
             if isinstance(m, torch.nn.Conv2d)]
    with torch.no_grad():
        discr(x)
    for h in hooks:
        h.remove()
    assert seen and all(0.25 <= s <= 0.75 for s in seen), "%s: positive pre-activations per convolution %s" % (what, seen)
    return min(seen), max(seen)


def adversarial_step(models, utils, ScreenSpaceShading, model, criterion, gen_optimizer, discr_optimizer, batch, opt, disc_steps):
    """mainVideoUnshaded.py:506-624 for one batch, statement by statement."""
    input, flow, target = batch
    B, T, Cout, Hhigh, Whigh = target.shape
    total_gt_score = total_pred_score = 0.0

    def frame_inputs(j, previous_output):
        if j == 0:
            previous_warped = utils.initialImage(input[:, 0], Cout, opt.initialImage, False, opt.upscale_factor)
            previous_warped_loss = target[:, 0]
            previous_input = F.interpolate(input[:, 0], size=(Hhigh, Whigh), mode=opt.upsample)
        else:
            previous_warped = models.VideoTools.warp_upscale(previous_output, flow[:, j - 1], opt.upscale_factor, special_mask=True)
            previous_warped_loss = previous_warped
            previous_input = F.interpolate(input[:, j - 1], size=(Hhigh, Whigh), mode=opt.upsample)
            previous_input = models.VideoTools.warp_upscale(previous_input, flow[:, j - 1], opt.upscale_factor, special_mask=True)
        flat = models.VideoTools.flatten_high(previous_warped, opt.upscale_factor)
        return torch.cat((input[:, j], flat), dim=1), previous_warped_loss, previous_input

    def feed_back(prediction):
        return torch.cat([torch.clamp(prediction[:, 0:1], -1, +1), ScreenSpaceShading.normalize(prediction[:, 1:4], dim=1),
                          torch.clamp(prediction[:, 4:5], 0, +1), torch.clamp(prediction[:, 5:6], 0, +1)], dim=1)

    for _ in range(disc_steps):                                   # DISCRIMINATOR (:508-566)
        discr_optimizer.zero_grad()
        gen_optimizer.zero_grad()
        loss, previous_output = 0, None
        for j in range(T):
            single_input, previous_warped_loss, previous_input = frame_inputs(j, previous_output)
            with torch.no_grad():
                prediction, _ = model(single_input)
            gt_prev_warped = models.VideoTools.warp_upscale(target[:, j - 1], flow[:, j - 1], opt.upscale_factor, special_mask=True)
            input_high = F.interpolate(input[:, j], size=(Hhigh, Whigh), mode=opt.upsample)
            disc_loss, gt_score, pred_score = criterion.train_discriminator(input_high, target[:, j], previous_input, gt_prev_warped,
                                                                            prediction, previous_warped_loss)
            loss += disc_loss
            total_gt_score += float(gt_score)
            total_pred_score += float(pred_score)
            previous_output = feed_back(prediction)
        loss.backward()
        discr_optimizer.step()
    discr_loss = loss.item()
    for _ in range(disc_steps):                                   # GENERATOR (:572-620; the loop count is disc_steps there too)
        discr_optimizer.zero_grad()
        gen_optimizer.zero_grad()
        loss, previous_output = 0, None
        for j in range(T):
            single_input, previous_warped_loss, previous_input = frame_inputs(j, previous_output)
            prediction, _ = model(single_input)
            input_high = F.interpolate(input[:, j], size=(Hhigh, Whigh), mode=opt.upsample)
            loss0, _ = criterion(target[:, j], prediction, input_high, previous_input, previous_warped_loss)
            loss += loss0
            previous_output = feed_back(prediction)
        loss.backward()
        gen_optimizer.step()
    return discr_loss, loss.item(), total_gt_score, total_pred_score


def main():
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    F.grid_sample = functools.partial(F.grid_sample, align_corners=True)
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "losses")):
        sys.exit("usage: make_gan_fixtures.py <reference checkout>/SuperresolutionNetwork")
    if "torchvision" not in sys.modules:
        try:
            import torchvision  # noqa: F401
        except ImportError:
            stub = types.ModuleType("torchvision")
            stub.models = types.ModuleType("torchvision.models")
            sys.modules["torchvision"], sys.modules["torchvision.models"] = stub, stub.models
    full = torch.full
    torch.full = lambda size, fill_value, *a, **k: full(size, float(fill_value) if "dtype" not in k else fill_value, *a, **k)
    sys.path.insert(0, sys.argv[1])
    import losses
    import models
    import utils
    from utils import ScreenSpaceShading

    out = {"weight_seed": np.int64(C.WEIGHT_SEED)}
    worst, logits_all = 0.0, []

    def note(what, v32, v64):
        nonlocal worst
        d = float(np.abs(np.asarray(v32, dtype=np.float64) - np.asarray(v64, dtype=np.float64)).max())
        print("%-46s fp32 vs fp64 %.2e" % (what, d))
        worst = max(worst, d)
        return d

    # ---- a: the discriminators
    builder = losses.LossBuilder(torch.device("cpu"))
    for k, (name, res, channels) in enumerate(C.DISCRIMINATOR_CASES):
        d32 = C.fill_state_dict(builder.build_discriminator(name, res, channels, None), C.WEIGHT_SEED)
        d64 = C.fill_state_dict(builder.build_discriminator(name, res, channels, None).double(), C.WEIGHT_SEED)
        x = C.discriminator_input(k)
        with torch.no_grad():
            y32, y64 = d32(x), d64(x.double())
        tag = "a%d" % k
        out[tag + "_keys"] = np.array(["%s:%s" % (key, ",".join(str(s) for s in t.shape)) for key, t in d32.state_dict().items()])
        out[tag + "_logits"] = y32.numpy()
        note("%s %s %d x %d, %d channels: logits" % (tag, name, res, res, channels), y32.numpy(), y64.numpy())
        print("    logits", y32.flatten().tolist(), "positive pre-activations %.2f .. %.2f" % check_signs(d32, x, tag))
        logits_all += y32.flatten().abs().tolist()

    # ---- b: the criterion
    def criterion_b(dtype):
        crit = losses.LossNetUnshaded(torch.device("cpu"), 5, 6, 16, 2, C.options(C.LOSSES_B, "enhanceNetLarge"))
        C.fill_criterion(crit)
        return crit.double() if dtype == torch.float64 else crit
    res_b = {}
    for dtype in (torch.float32, torch.float64):
        crit = criterion_b(dtype)
        fwd, discr = C.criterion_inputs()
        fwd, discr = [t.to(dtype) for t in fwd], [t.to(dtype) for t in discr]
        fwd[1].requires_grad_(True)
        fwd[4].requires_grad_(True)
        total, values = crit(*fwd)
        total.backward()
        dl, gs, ps = crit.train_discriminator(*discr)
        res_b[dtype] = dict(total=total.item(), values=values, gpred=fwd[1].grad.numpy(), gprev=fwd[4].grad.numpy(),
                            discr=np.array([dl.item(), float(gs), float(ps)]))
        if dtype == torch.float32:
            for name in ("discriminator", "temp_discriminator", "spatial_discriminator"):
                with torch.no_grad():
                    probe = C.uniform(250, 2, getattr(crit, name).input_channels, 16, 16)
                check_signs(getattr(crit, name), probe, "b " + name)
    r32, r64 = res_b[torch.float32], res_b[torch.float64]
    keys = sorted(r32["values"], key=str)
    out["b_total"] = np.float64(r32["total"])
    out["b_value_keys"] = np.array([str(k) for k in keys])
    out["b_values"] = np.array([r32["values"][k] for k in keys], dtype=np.float64)
    out["b_grad_pred"], out["b_grad_prev"], out["b_train_discr"] = r32["gpred"], r32["gprev"], r32["discr"]
    note("b total", r32["total"], r64["total"])
    note("b values", out["b_values"], [r64["values"][k] for k in keys])
    note("b gradient of pred", r32["gpred"], r64["gpred"])
    note("b gradient of prev_pred_warped", r32["gprev"], r64["gprev"])
    note("b train_discriminator", r32["discr"], r64["discr"])
    print("    b values", dict(zip(out["b_value_keys"].tolist(), out["b_values"].tolist())), "train_discriminator", r32["discr"].tolist())

    # ---- c: one adversarial step
    res_c = {}
    for dtype in (torch.float32, torch.float64):
        opt = C.options(C.LOSSES_C, "enhanceNetSmall")
        model = C.fill_state_dict(models.createNetwork('EnhanceNet', 4, 5 + 6 * 16, [0, 1, 2, 3, 4], 6, opt), C.WEIGHT_SEED + 10, gain=True)
        crit = C.fill_criterion(losses.LossNetUnshaded(torch.device("cpu"), 5, 6, 16, 2, opt))
        if dtype == torch.float64:
            model, crit = model.double(), crit.double()
        model.train()
        crit.discr_train()
        gen_optimizer = torch.optim.SGD(model.parameters(), lr=C.LR_GEN)
        discr_optimizer = torch.optim.SGD(crit.get_discr_parameters(), lr=C.LR_DISCR)
        before = C.named_parameters(model, crit)
        batch = tuple(t.to(dtype) for t in C.clip_batch())
        returns = adversarial_step(models, utils, ScreenSpaceShading, model, crit, gen_optimizer, discr_optimizer, batch, opt, C.DISC_STEPS)
        res_c[dtype] = (np.array(returns), C.parameter_changes(before, C.named_parameters(model, crit)))
    (ret32, ch32), (ret64, ch64) = res_c[torch.float32], res_c[torch.float64]
    note("c returns (discr, gen, gt score, pred score)", ret32, ret64)
    print("    c returns", ret32.tolist())
    names = list(ch32)
    out["c_returns"] = ret32
    out["c_names"] = np.array(names)
    out["c_max_change"] = np.array([ch32[n][1] for n in names])
    rel = []
    for n in names:
        out["c_change." + n] = ch32[n][0].astype(np.float32)
        assert ch32[n][1] > 0, "parameter %s did not change" % n
        rel.append(float(np.abs(ch32[n][0] - ch64[n][0]).max() / ch64[n][1]))
        print("    %-46s largest change %.3e, fp32 vs fp64 relative %.2e" % (n, ch32[n][1], rel[-1]))
    out["c_cpu32_vs_fp64"] = np.array(rel)
    out["c_lr"] = np.array([C.LR_GEN, C.LR_DISCR])

    strong = float(np.mean(np.array(logits_all) >= 0.5))
    assert strong >= 0.25, "only %.0f %% of the logits have |logit| >= 0.5" % (100 * strong)
    assert worst <= PREMISE, "the reference itself is %g from fp64" % worst
    np.savez_compressed(OUT, **out)
    assert os.path.getsize(OUT) < 1000000, os.path.getsize(OUT)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; worst fp32-fp64 distance %.2e; |logit| >= 0.5: %.0f %%" % (worst, 100 * strong))


if __name__ == "__main__":
    main()
