"""Adversarial training step on the HIP path: the three routes of the discriminators' stride-2 convolutions, interleaved on one box,
beside the plain (non-adversarial) training step.

Batch: the reference's, 16 clips x 10 frames, 32^2 -> 128^2; generator: the unshaded EnhanceNet of ``bench.py --mode train``; criterion:
the README loss recipe plus ``adv:all:0.01`` with ``enhanceNetLarge`` (the trainer's default) or ``enhanceNetSmall``.  Everything runs
eagerly, except the row that ``--graph`` adds.  Routes (``ops.CONV_S2_ROUTE``, ``--routes``):
  kernel    conv3x3s2_fwd_kernel / conv3x3s2_dgrad_kernel / conv3x3s2_wgrad_kernel (csrc/sr_conv_stride2.hip)
  embedded  the layer as a stride-1 3x3 layer over pixel_unshuffle(x, 2), 9 of 36 taps live, on ``ops.conv3x3`` (4x the matrix work)
  torch     PyTorch's convolution under autograd
Timed per route, ``--rounds`` rounds of ``--steps`` each, the routes interleaved: the discriminator phase alone (one discriminator
step: generator without gradients, discriminators forward and backward, Adam), the generator phase alone (one generator step) and the
whole ``train.adversarial_step`` (two of each).  ``plain`` is ``train.train_step`` of the same generator with the recipe's criterion,
eager, on the same box.  Then ONE whole step of the kernel route under ``ops.profile_enable``: per library kernel launches and
milliseconds; the time between the step's bracketing events that no library kernel accounts for is the torch side (input assembly,
the two Linear layers, Adam, element-wise autograd); the Linear layers' share of it is measured on their own, forward and backward at
the step's batch, times the step's calls.

``--fused-input 0`` assembles the discriminators' inputs with torch operators (``ops.DISCR_INPUT_FUSED = False``), 1 (the default)
with ``discr_input_fwd_kernel`` / ``discr_input_bwd_kernel``: two runs of this tool are the A/B of that switch.  ``--graph`` adds the
whole step of the kernel route replayed from ``train.GraphedAdversarialStep`` (its own generator, criterion and capturable Adams),
timed in every round beside the eager ones.  The profiled step's table gives the two assembly kernels' bytes per second against the
bytes they have to move (forward: every operand read once, the output written once; backward: the output's gradient and the operands
read, the two gradients written).

Usage: python tools/bench_gan_train.py [--steps 3] [--rounds 2] [--configs enhanceNetLarge,enhanceNetSmall] [--routes kernel,embedded,torch]
                                       [--fused-input {0,1}] [--graph] [--out profiles/gan_train.md]"""
import argparse
import contextlib
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from isosurfacesuperresolution_amd import losses, models, ops, train

ROUTES = ("kernel", "embedded", "torch")
B, T, CROP, BLOCKS = 16, 10, 32, 10
RECIPE = "l1:mask:1,l1:ao:1,l1:normal:10,l1:depth:10,temp-l2:color:0.1"


def options(loss_spec, discriminator):
    return argparse.Namespace(upsample='bilinear', reconType='residual', useBN=False, numResidualLayers=BLOCKS, losses=loss_spec,
                              discriminator=discriminator, lossAO=0.0, lossAmbient=0.1, lossDiffuse=0.9, lossSpecular=0.0)


def make_batch():
    g = torch.Generator().manual_seed(1000)
    inp = torch.rand(B, T, 5, CROP, CROP, generator=g); inp[:, :, 0] = inp[:, :, 0] * 2 - 1
    flow = (torch.rand(B, T, 2, CROP, CROP, generator=g) - 0.5) * 0.05
    tgt = torch.rand(B, T, 6, 4 * CROP, 4 * CROP, generator=g); tgt[:, :, 0] = tgt[:, :, 0] * 2 - 1
    return tuple(t.cuda() for t in (inp, flow, tgt))


def build(discriminator, capturable=False):
    """Generator, criterion and optimizers of one configuration (discriminator None: the plain recipe)."""
    opt = options(RECIPE + (",adv:all:0.01" if discriminator else ""), discriminator)
    torch.manual_seed(124)
    with contextlib.redirect_stdout(sys.stderr):
        net = models.createNetwork('EnhanceNet', 4, 101, [0, 1, 2, 3, 4], 6, opt).cuda()
        crit = losses.LossNetUnshaded('cuda', 5, 6, 4 * CROP, CROP // 2, opt).cuda()
    st = {"net": net, "crit": crit}
    if discriminator:
        st["gen_opt"], st["discr_opt"], _, _ = train.make_adversarial_optimizers(net, crit, capturable=capturable)
    else:
        st["opt"], _ = train.make_optimizer(net)
    return st


def discriminator_phase(st, batch):
    st["discr_opt"].zero_grad()
    loss, _, _ = train.discriminator_clip_loss(st["net"], st["crit"], *batch, initial_image="zero")
    train.backward(loss)
    st["discr_opt"].step()


def generator_phase(st, batch):
    params = st["crit"].get_discr_parameters()
    for p in params:
        p.requires_grad_(False)
    try:
        st["gen_opt"].zero_grad()
        loss, _ = train.clip_loss(st["net"], st["crit"], *batch, initial_image="zero")
        train.backward(loss)
        st["gen_opt"].step()
    finally:
        for p in params:
            p.requires_grad_(True)


def whole_step(st, batch):
    train.adversarial_step(st["net"], st["crit"], st["gen_opt"], st["discr_opt"], batch, 2, initial_image="zero")


def plain_step(st, batch):
    train.train_step(st["net"], st["crit"], st["opt"], batch, initial_image="zero")


def graphed_step(st, batch):
    st["graphed"](batch)


def timed(fn, st, batch, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn(st, batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def profile_step(st, batch):
    """One whole step of the current route: ({kernel: (launches, ms)}, ms between the bracketing events)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ops.profile_enable(True)
    try:
        e0.record()
        whole_step(st, batch)
        e1.record()
        torch.cuda.synchronize()
        records = ops.profile_records()
    finally:
        ops.profile_enable(False)
    kernels = {}
    for name, _, ms in records:
        n, t = kernels.get(name, (0, 0.0))
        kernels[name] = (n + 1, t + ms)
    return kernels, e0.elapsed_time(e1)


def linear_share(st, calls, rows):
    """ms of the classifier (Linear, LeakyReLU, Linear) forward and backward at ``rows`` images, times ``calls``."""
    cls = st["crit"].discriminator.classifier
    x = torch.randn(rows, cls[0].in_features, device="cuda", requires_grad=True)
    for _ in range(2):
        cls(x).sum().backward()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        cls(x).sum().backward()
    e1.record()
    torch.cuda.synchronize()
    for p in cls.parameters():
        p.grad = None
    return e0.elapsed_time(e1) / 10 * calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--configs", default="enhanceNetLarge,enhanceNetSmall")
    ap.add_argument("--routes", default=",".join(ROUTES))
    ap.add_argument("--fused-input", type=int, choices=(0, 1), default=1)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    routes = tuple(args.routes.split(","))
    assert routes and all(r in ROUTES for r in routes), routes
    ops.DISCR_INPUT_FUSED = bool(args.fused_input)
    batch = make_batch()
    plain = build(None)
    lines = ["# Adversarial training step: the routes of the stride-2 convolutions", "",
             "`tools/bench_gan_train.py --steps %d --rounds %d`: %d clips x %d frames, %d^2 -> %d^2, unshaded EnhanceNet of %d blocks, README "
             "recipe + `adv:all:0.01`, eager, Adam; routes interleaved on one MI355X (%s).  Discriminator inputs assembled by %s.  Milliseconds "
             "per call, best of the rounds (all rounds in brackets)." %
             (args.steps, args.rounds, B, T, CROP, 4 * CROP, BLOCKS, torch.cuda.get_device_name(0),
              "the assembly kernels (`--fused-input 1`)" if args.fused_input else "torch operators (`--fused-input 0`)"), ""]
    phases = (("discriminator phase (1 step)", discriminator_phase), ("generator phase (1 step)", generator_phase),
              ("whole step (2 + 2)", whole_step))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for discriminator in args.configs.split(","):
            st = build(discriminator)
            times = {(route, name): [] for route in routes for name, _ in phases}
            times_plain, times_graph = [], []
            for route in routes:                                               # one untimed call of everything per route
                ops.CONV_S2_ROUTE = route
                whole_step(st, batch)
            plain_step(plain, batch)
            graphed = None
            if args.graph:
                ops.CONV_S2_ROUTE = "kernel"
                graphed = build(discriminator, capturable=True)
                graphed["graphed"] = train.GraphedAdversarialStep(graphed["net"], graphed["crit"], graphed["gen_opt"], graphed["discr_opt"], batch,
                                                                  2, warmup=1, initial_image="zero")
                graphed_step(graphed, batch)
            for _ in range(args.rounds):
                for route in routes:
                    ops.CONV_S2_ROUTE = route
                    for name, fn in phases:
                        times[(route, name)].append(timed(fn, st, batch, args.steps))
                times_plain.append(timed(plain_step, plain, batch, args.steps))
                if graphed is not None:
                    times_graph.append(timed(graphed_step, graphed, batch, args.steps))
                sys.stderr.write("%s: round done\n" % discriminator)
                sys.stderr.flush()
            lines += ["## %s" % discriminator, "", "| route | " + " | ".join(name for name, _ in phases) + " |", "|---|---|---|---|"]
            for route in routes:
                lines.append("| %s | " % route + " | ".join("%.1f (%s)" % (min(times[(route, name)]), ", ".join("%.1f" % m for m in times[(route, name)]))
                                                           for name, _ in phases) + " |")
            lines += ["", "Plain `train_step` (no adversarial term, eager) on the same box: %.1f ms (%s)." %
                      (min(times_plain), ", ".join("%.1f" % m for m in times_plain))]
            if graphed is not None:
                lines += ["Whole step (2 + 2) of the `kernel` route replayed from `train.GraphedAdversarialStep`: %.1f ms (%s)." %
                          (min(times_graph), ", ".join("%.1f" % m for m in times_graph))]
                del graphed
            best = min(routes, key=lambda r: min(times[(r, phases[2][0])]))
            lines += ["Fastest route for the whole step: **%s**." % best, ""]
            ops.CONV_S2_ROUTE = "kernel"
            kernels, wall = profile_step(st, batch)
            lib_ms = sum(ms for _, ms in kernels.values())
            s2 = sum(ms for k, (_, ms) in kernels.items() if k.startswith("conv3x3s2"))
            # discriminator evaluations of a whole step: 2 discriminator steps x T frames x 2 inputs, 2 generator steps x T frames
            lin = linear_share(st, 2 * T * 2 + 2 * T, B)
            lines += ["One whole step of the `kernel` route under the per-dispatch profiler: %.1f ms between its bracketing events, %.1f ms in "
                      "library kernels, of which %.1f ms (%.1f %% of the step) in the stride-2 kernels; %.1f ms (%.1f %%) on the torch side "
                      "(input assembly, Linear layers, Adam, element-wise autograd, launch gaps), of which the two Linear layers, measured "
                      "on their own (forward and backward at %d images x %d calls): %.1f ms (%.1f %%)." %
                      (wall, lib_ms, s2, 100 * s2 / wall, wall - lib_ms, 100 * (wall - lib_ms) / wall, B, 2 * T * 2 + 2 * T, lin, 100 * lin / wall), "",
                      "| kernel | launches | ms | % of the step |", "|---|---|---|---|"]
            for name, (n, ms) in sorted(kernels.items(), key=lambda kv: -kv[1][1]):
                lines.append("| `%s` | %d | %.3f | %.1f |" % (name, n, ms, 100 * ms / wall))
            lines.append("")
            # bytes the assembly kernels have to move at this batch (adv: 5 + 5 + 6 + 6 channels in, 26 out; backward: 26 + 12 in, 12 out)
            plane_bytes = 4 * B * (4 * CROP) ** 2
            for name, moved in (("discr_input_fwd_kernel", (22 + 26) * plane_bytes), ("discr_input_bwd_kernel", (26 + 12 + 12) * plane_bytes)):
                if name in kernels:
                    n, ms = kernels[name]
                    lines.append("`%s`: %d launches, %.1f us each, %.1f MB per launch (all operands present; a frame without a gradient for "
                                 "`prev` moves less): %.2f TB/s." % (name, n, 1e3 * ms / n, moved / 1e6, moved * n / (ms * 1e-3) / 1e12))
            lines.append("")
            del st
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
