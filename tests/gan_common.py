"""What the adversarial-training tests and tests/golden/make_gan_fixtures.py share: the weight rule, the inputs and the options of the
recorded cases.  Nothing here is stored in the fixture: both sides draw weights and inputs from ``numpy.random.RandomState`` streams.

Weights (``fill_state_dict``), for every key in ``state_dict()`` order, n = standard_normal(shape):
    convolution weight [a, b, 3, 3]    sqrt(2 / (9 b)) * n        (He scale on the inputs)
    Linear weight [a, b]               2 * n / sqrt(b)
    every bias                         0.05 * n
and, for the GENERATOR of case c only (``gain=True``), 0.25 times that on the second convolution of every residual block
(``blocks.<k>.2.weight``): the reference's EnhanceNet always has ten blocks (it has no option for their number), and ten He-scaled
residual additions in a row leave nothing of fp32 after two SGD steps.
The reference's own initialisation (Linear N(0, 0.01), zero biases) gives logits near 0.005 and a loss of ln 2 whatever the convolutions
compute; with this rule the logits spread over |logit| 0.5 .. 4 and every convolution has both signs among its pre-activations.

Parameter changes of case c are recorded as SAMPLES (``sample_indices``: every element of a tensor of at most 4096, else 4096-odd
elements at an odd stride) together with each tensor's largest |change|: the two networks have 0.9 million parameters, the fixture
stays under 1 MB."""
import argparse

import numpy as np
import torch

WEIGHT_SEED = 61
SAMPLES = 4096

# case a: (discriminator, resolution, input channels), N = 3
DISCRIMINATOR_CASES = [("enhanceNetSmall", 16, 26), ("enhanceNetSmall", 32, 13), ("enhanceNetLarge", 16, 16), ("enhanceNetLarge", 32, 26)]
LOSSES_B = "l1:mask:1,temp-l2:color:0.1,adv:all:0.5,tgan:all:0.25,sgan:all:0.125"
LOSSES_C = "l1:mask:1,temp-l2:color:0.1,adv:all:0.5"
LR_GEN, LR_DISCR = 1e-3, 5e-3          # case c, torch.optim.SGD on both sides (Adam's first step is the sign of the gradient)
DISC_STEPS = 2


def options(losses, discriminator, residual_layers=10):
    return argparse.Namespace(upsample='bilinear', reconType='residual', useBN=False, numResidualLayers=residual_layers, losses=losses,
                              discriminator=discriminator, lossAO=0.0, lossAmbient=0.1, lossDiffuse=0.9, lossSpecular=0.0,
                              upscale_factor=4, initialImage='zero')


def fill_state_dict(module, seed, gain=False):
    rs = np.random.RandomState(seed)
    sd = module.state_dict()
    for key, t in sd.items():
        n = rs.standard_normal(tuple(t.shape))
        if t.dim() == 4:
            v = n * np.sqrt(2.0 / (9.0 * t.shape[1])) * (0.25 if gain and key.startswith("blocks.") and key.endswith(".2.weight") else 1.0)
        elif t.dim() == 2:
            v = n * (2.0 / np.sqrt(t.shape[1]))
        else:
            v = 0.05 * n
        sd[key] = torch.from_numpy(v).to(t.dtype)
    module.load_state_dict(sd)
    return module


def fill_criterion(criterion, seed=WEIGHT_SEED):
    """The criterion's discriminators, each from its own stream (seed, seed + 1, seed + 2 in attribute order)."""
    for k, name in enumerate(('discriminator', 'temp_discriminator', 'spatial_discriminator')):
        if hasattr(criterion, name):
            fill_state_dict(getattr(criterion, name), seed + k)
    return criterion


def uniform(seed, *shape):
    """fp32 values uniform in [-1, 1)."""
    return torch.from_numpy(np.random.RandomState(seed).uniform(-1.0, 1.0, shape).astype(np.float32))


def discriminator_input(index):
    _, res, channels = DISCRIMINATOR_CASES[index]
    return uniform(100 + index, 3, channels, res, res)


def criterion_inputs():
    """Case b, B = 2 at 16 x 16: gt, pred, input, prev_input_warped, prev_pred_warped of ``forward`` and the six of ``train_discriminator``."""
    fwd = [uniform(200 + k, 2, c, 16, 16) for k, c in enumerate((6, 6, 5, 5, 6))]
    discr = [uniform(210 + k, 2, c, 16, 16) for k, c in enumerate((5, 6, 5, 6, 6, 6))]
    return fwd, discr


def clip_batch():
    """Case c, B = 2, T = 3, 4 x 4 -> 16 x 16: (input [B, T, 5, 4, 4], flow [B, T, 2, 4, 4] of at most 0.1 of the image, target)."""
    return uniform(300, 2, 3, 5, 4, 4), uniform(301, 2, 3, 2, 4, 4) * 0.1, uniform(302, 2, 3, 6, 16, 16)


def sample_indices(numel):
    if numel <= SAMPLES:
        return np.arange(numel)
    return np.arange(0, numel, (numel // SAMPLES) | 1)


def parameter_changes(before, after):
    """{name: (samples of after - before, largest |after - before|)} for two ``{name: tensor}`` dicts."""
    out = {}
    for name, b in before.items():
        d = (after[name].detach().double().cpu() - b.double().cpu()).reshape(-1).numpy()
        out[name] = (d[sample_indices(d.size)], float(np.abs(d).max()))
    return out


def named_parameters(model, criterion):
    """{'gen.<key>' | '<discriminator attribute>.<key>': detached clone} of everything an adversarial step changes."""
    out = {"gen." + k: v.detach().clone() for k, v in model.named_parameters()}
    for name in ('discriminator', 'temp_discriminator', 'spatial_discriminator'):
        if hasattr(criterion, name):
            out.update({name + "." + k: v.detach().clone() for k, v in getattr(criterion, name).named_parameters()})
    return out


# ---- the checks the CPU and the GPU tests share (tests/test_gan_cpu.py, tests/test_gan_gpu.py) ------------------------------------------
def reference():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gan_reference.npz"))


def check_discriminators(device):
    """Case a: keys and shapes equal the fixture's, logits within 1e-4."""
    from isosurfacesuperresolution_amd import losses
    ref = reference()
    builder = losses.LossBuilder(device)
    for k, (name, res, channels) in enumerate(DISCRIMINATOR_CASES):
        d = fill_state_dict(builder.build_discriminator(name, res, channels, None), WEIGHT_SEED).to(device)
        assert (d.resolution, d.input_channels) == (res, channels)
        assert ["%s:%s" % (key, ",".join(str(s) for s in t.shape)) for key, t in d.state_dict().items()] == ref["a%d_keys" % k].tolist()
        with torch.no_grad():
            y = d(discriminator_input(k).to(device))
        err = np.abs(y.cpu().numpy() - ref["a%d_logits" % k]).max()
        print("a%d %s %d: logits within %.2e" % (k, name, res, err))
        assert y.shape == (3, 1) and err <= 1e-4, (name, res, err)


def make_criterion(device, losses_spec=LOSSES_B, discriminator="enhanceNetLarge"):
    from isosurfacesuperresolution_amd import losses
    return fill_criterion(losses.LossNetUnshaded(device, 5, 6, 16, 2, options(losses_spec, discriminator))).to(device)


def check_criterion(device, fused=True):
    """Case b: total, values, gradients of pred and prev_pred_warped, train_discriminator's returns, all within 1e-4."""
    ref = reference()
    crit = make_criterion(device)
    crit.fused = fused
    fwd, discr = criterion_inputs()
    fwd, discr = [t.to(device) for t in fwd], [t.to(device) for t in discr]
    fwd[1].requires_grad_(True)
    fwd[4].requires_grad_(True)
    total, values = crit(*fwd)
    total.backward()
    assert abs(total.item() - float(ref["b_total"])) <= 1e-4, (total.item(), float(ref["b_total"]))
    assert sorted(str(k) for k in values) == ref["b_value_keys"].tolist()
    got = np.array([float(values[k]) for k in sorted(values, key=str)])
    print("b values within %.2e, total within %.2e" % (np.abs(got - ref["b_values"]).max(), abs(total.item() - float(ref["b_total"]))))
    assert np.abs(got - ref["b_values"]).max() <= 1e-4, (got, ref["b_values"])
    for name, t in (("b_grad_pred", fwd[1]), ("b_grad_prev", fwd[4])):
        err, bar = np.abs(t.grad.cpu().numpy() - ref[name]).max(), 1e-4 * max(1.0, np.abs(ref[name]).max())
        print("%s within %.2e (bar %.1e)" % (name, err, bar))
        assert err <= bar, (name, err)
    for p in crit.get_discr_parameters():                        # (the generator-side pass left gradients on the discriminators)
        p.grad = None
    dl, gs, ps = crit.train_discriminator(*discr)
    got = np.array([dl.item(), float(gs), float(ps)])
    assert np.abs(got - ref["b_train_discr"]).max() <= 1e-4, (got, ref["b_train_discr"])
    return crit


def check_step(device):
    """Case c through ``train.adversarial_step``: returns within 1e-4; every parameter's change within four times the fixture's own
    fp32-against-fp64 distance for that tensor (a second, different summation order of the same fp32 sums), not below 1e-5, relative to
    the tensor's largest change.  -> [(name, error, bar)]."""
    from isosurfacesuperresolution_amd import models, train
    ref = reference()
    opt = options(LOSSES_C, "enhanceNetSmall")
    model = fill_state_dict(models.createNetwork('EnhanceNet', 4, 5 + 6 * 16, [0, 1, 2, 3, 4], 6, opt), WEIGHT_SEED + 10, gain=True).to(device)
    crit = make_criterion(device, LOSSES_C, "enhanceNetSmall")
    model.train()
    crit.discr_train()
    gen_optimizer = torch.optim.SGD(model.parameters(), lr=LR_GEN)
    discr_optimizer = torch.optim.SGD(crit.get_discr_parameters(), lr=LR_DISCR)
    before = named_parameters(model, crit)
    batch = tuple(t.to(device) for t in clip_batch())
    returns = train.adversarial_step(model, crit, gen_optimizer, discr_optimizer, batch, DISC_STEPS, initial_image="zero")
    print("c returns", returns, "reference", ref["c_returns"].tolist())
    assert np.abs(np.array(returns) - ref["c_returns"]).max() <= 1e-4, (returns, ref["c_returns"])
    assert all(p.requires_grad for p in crit.get_discr_parameters())
    changes = parameter_changes(before, named_parameters(model, crit))
    assert list(changes) == ref["c_names"].tolist()
    rows = []
    for k, name in enumerate(changes):
        err = float(np.abs(changes[name][0] - ref["c_change." + name]).max() / ref["c_max_change"][k])
        rows.append((name, err, max(1e-5, 4.0 * float(ref["c_cpu32_vs_fp64"][k]))))
        print("%-44s change within %.2e of the reference's (bar %.2e, relative to %.2e)" % (rows[-1] + (ref["c_max_change"][k],)))
    bad = [r for r in rows if r[1] > r[2]]
    assert not bad, bad
    return rows
