"""Training step of a TecoGAN on the HIP path: the three routes of its two transposed convolutions, interleaved on one box.

Configuration: that of ``bench.py --mode train`` (16 clips x 10 frames, 32^2 -> 128^2, README loss recipe, the whole step in one HIP
graph, flat Adam) with a direct unshaded TecoGAN of 10 blocks.  Routes (``ops.CONVT_TRAIN_ROUTE``):
  A  "torch"     PyTorch's transposed convolution under autograd (the route before the backward kernels existed)
  B  "embedded"  forward, data gradient and weight gradient as the zero-embedded 64 -> 256 3x3 layer on the convolution's kernels
  C  "kernel"    convt3x3s2_split_kernel forward, convt3x3s2_dgrad_split_kernel, the weight gradient embedded (the default)
Three rounds of ``--steps`` replays each, A B C A B C ...; then ONE eager step of B and of C under ``ops.profile_enable`` for the
per-kernel table and the launches of the layers' data and weight gradients (a replayed graph has no per-dispatch events).

Usage: python tools/bench_tecogan_train.py [--steps 20] [--rounds 3] [--out profiles/tecogan_train.md]"""
import argparse
import contextlib
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from isosurfacesuperresolution_amd import losses, models, ops, train

ROUTES = (("A", "torch"), ("B", "embedded"), ("C", "kernel"))
B, T, CROP, BLOCKS = 16, 10, 32, 10


def build(route):
    opt = argparse.Namespace(upsample='bilinear', reconType='direct', useBN=False, numResidualLayers=BLOCKS,
                             losses="l1:mask:1,l1:ao:1,l1:normal:10,l1:depth:10,temp-l2:color:0.1",
                             lossAO=0.0, lossAmbient=0.1, lossDiffuse=0.9, lossSpecular=0.0)
    torch.manual_seed(124)
    with contextlib.redirect_stdout(sys.stderr):
        net = models.createNetwork('TecoGAN', 4, 101, [0, 1, 2, 3, 4], 6, opt).cuda()
        crit = losses.LossNetUnshaded('cuda', 5, 6, 4 * CROP, CROP // 2, opt).cuda()
    optim, _ = train.make_optimizer(net, capturable=True, flat=True)
    g = torch.Generator().manual_seed(1000)
    inp = torch.rand(B, T, 5, CROP, CROP, generator=g); inp[:, :, 0] = inp[:, :, 0] * 2 - 1
    flow = (torch.rand(B, T, 2, CROP, CROP, generator=g) - 0.5) * 0.05
    tgt = torch.rand(B, T, 6, 4 * CROP, 4 * CROP, generator=g); tgt[:, :, 0] = tgt[:, :, 0] * 2 - 1
    batch = tuple(t.cuda() for t in (inp, flow, tgt))
    ops.CONVT_TRAIN_ROUTE = route
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        step = train.GraphedTrainStep(net, crit, optim, batch, initial_image="zero")
    return {"net": net, "crit": crit, "optim": optim, "batch": batch, "step": step}


def profile_eager_step(state, route):
    """One eager step under the per-dispatch profiler: {kernel: (launches, ms)}, and the launches made inside the transposed
    convolutions' data-gradient and weight-gradient calls, keyed by (what, low-resolution height)."""
    lib = ops._sr()
    spans = []

    def spanned(what, fn, height):
        def wrapper(*a, **kw):
            c0 = lib.isrProfileCount()
            out = fn(*a, **kw)
            spans.append((what, height(*a), c0, lib.isrProfileCount()))
            return out
        return wrapper

    saved = (ops._convt_data_grad, ops._convt_data_grad_embedded, ops._convt_weight_grad)
    ops._convt_data_grad = spanned("data gradient", saved[0], lambda g, *a: g.shape[2])
    ops._convt_data_grad_embedded = spanned("data gradient", saved[1], lambda g, *a: g.shape[2])
    ops._convt_weight_grad = spanned("weight gradient", saved[2], lambda xs, *a: xs[0].shape[2])
    ops.CONVT_TRAIN_ROUTE = route
    torch.cuda.synchronize()
    ops.profile_enable(True)
    try:
        train.train_step(state["net"], state["crit"], state["optim"], state["batch"], initial_image="zero")
        torch.cuda.synchronize()
        records = ops.profile_records()
    finally:
        ops.profile_enable(False)
        ops._convt_data_grad, ops._convt_data_grad_embedded, ops._convt_weight_grad = saved
    kernels = {}
    for name, _, ms in records:
        n, t = kernels.get(name, (0, 0.0))
        kernels[name] = (n + 1, t + ms)
    layers = {}
    for what, h, c0, c1 in spans:
        n, t, names = layers.get((what, h), (0, 0.0, set()))
        layers[(what, h)] = (n + (c1 - c0), t + sum(r[2] for r in records[c0:c1]), names | {r[0] for r in records[c0:c1]})
    return kernels, layers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    states = {}
    for tag, route in reversed(ROUTES):
        t0 = time.perf_counter()
        states[tag] = build(route)
        sys.stderr.write("route %s (%s): warmed up and captured in %.1f s\n" % (tag, route, time.perf_counter() - t0))
        sys.stderr.flush()
    times = {tag: [] for tag, _ in ROUTES}
    for tag, _ in ROUTES:                                                  # two replays each before the first timed round
        for _ in range(2):
            states[tag]["step"](states[tag]["batch"])
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for tag, _ in ROUTES:
            st = states[tag]
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss = st["step"](st["batch"])
            torch.cuda.synchronize()
            times[tag].append((time.perf_counter() - t0) / args.steps * 1e3)
            st["loss"] = float(loss)
    lines = ["# TecoGAN training step: the routes of the transposed convolutions", "",
             "`tools/bench_tecogan_train.py --steps %d --rounds %d`: %d clips x %d frames, %d^2 -> %d^2, direct unshaded TecoGAN of %d blocks, "
             "one HIP graph, flat Adam; rounds interleaved A B C on one MI355X (%s)." % (args.steps, args.rounds, B, T, CROP, 4 * CROP, BLOCKS,
                                                                                    torch.cuda.get_device_name(0)), "",
             "| route | ms per step, by round | best | clips/s (best) | loss after the last step |", "|---|---|---|---|---|"]
    names = {"A": "A: PyTorch's transposed convolution under autograd", "B": "B: everything embedded (64 -> 256 3x3)",
             "C": "C: forward and data-gradient kernels, weight gradient embedded"}
    for tag, _ in ROUTES:
        ms = times[tag]
        lines.append("| %s | %s | %.2f | %.0f | %.5f |" % (names[tag], ", ".join("%.2f" % m for m in ms), min(ms), B / min(ms) * 1e3, states[tag]["loss"]))
    profiles = {tag: profile_eager_step(states[tag], route) for tag, route in ROUTES if tag != "A"}
    for tag in ("B", "C"):
        kernels, layers = profiles[tag]
        lines += ["", "## Route %s: launches with per-dispatch events in one eager step" % tag, "", "| kernel | launches | ms |", "|---|---|---|"]
        for name, (n, ms) in sorted(kernels.items(), key=lambda kv: -kv[1][1]):
            lines.append("| `%s` | %d | %.3f |" % (name, n, ms))
        lines += ["", "| transposed-convolution layer | launches | ms per step | ms per launch | kernels |", "|---|---|---|---|---|"]
        for (what, h), (n, ms, used) in sorted(layers.items()):
            lines.append("| %s, %d^2 -> %d^2 | %d | %.3f | %.4f | %s |" % (what, h, 2 * h, n, ms, ms / max(n, 1), ", ".join("`%s`" % u for u in sorted(used))))
    wg = sum(ms for (what, _), (_, ms, _) in profiles["C"][1].items() if what == "weight gradient")
    lines += ["", "Embedded weight gradient of the two layers on route C: %.3f ms of kernel time per step = %.1f %% of the %.2f ms step." %
              (wg, 100 * wg / min(times["C"]), min(times["C"]))]
    for h in (CROP, 2 * CROP):
        b, c = profiles["B"][1].get(("data gradient", h)), profiles["C"][1].get(("data gradient", h))
        if b and c:
            lines.append("Data gradient at %d^2 -> %d^2, per launch: embedded %.4f ms, `convt3x3s2_dgrad_split_kernel` %.4f ms (%.2fx)." %
                         (h, 2 * h, b[1] / b[0], c[1] / c[0], (b[1] / b[0]) / (c[1] / c[0])))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
