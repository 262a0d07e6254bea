"""Training a batch-norm EnhanceNet (``useBN``: 20 BatchNorm2d layers in the ten residual blocks, 101 in, 6 out) on the HIP path: one
optimisation step of an unshaded clip through ``train.clip_loss`` -- B = 16 clips of T = 10 frames, 32 x 32 -> 128 x 128 crops, the
unshaded L1 / temporal recipe, Adam -- eager (``train.train_step``'s sequence) and captured in a HIP graph
(``train.GraphedTrainStep``), with the batch-norm layers on the kernels of csrc/sr_batchnorm.hip (``ops.BATCH_NORM_KERNELS = True``)
and, for comparison, on PyTorch's operator (``False``; the convolutions run on the HIP training kernels either way).

    python tools/bench_bn_train.py [--steps 5] [--rounds 3] [--warmup 2] [--clips 16] [--frames 10]

Timing: wall clock around --steps steps between two device synchronisations, the four forms INTERLEAVED (one block of steps of each
per round), every round listed.  Launches: one eager step under ``ops.profile_enable`` -- the dispatches of THIS PACKAGE's kernels
per step and their device milliseconds by kernel name (``ops.profile_records()``; PyTorch's own launches, which is what the operator
consists of, are not in those records: its column shows what is left on the package's kernels).  Prints one JSON line."""
import argparse
import contextlib
import copy
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LOW, HIGH, PAD = 32, 128, 16
RECIPE = "l1:mask:1,l1:ao:1,l1:normal:10,l1:depth:10,temp-l2:color:0.1"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--frames", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bn_train.py measures on the GPU"
    from isosurfacesuperresolution_amd import losses, models, ops, train
    B, T = args.clips, args.frames
    opt = argparse.Namespace(upsample='bilinear', reconType='residual', useBN=True, numResidualLayers=10, losses=RECIPE,
                             lossAO=0.0, lossAmbient=0.1, lossDiffuse=0.9, lossSpecular=0.0)
    g = torch.Generator().manual_seed(0)
    inp = torch.rand(B, T, 5, LOW, LOW, generator=g); inp[:, :, 0] = inp[:, :, 0] * 2 - 1
    flow = (torch.rand(B, T, 2, LOW, LOW, generator=g) - 0.5) * 0.05
    tgt = torch.rand(B, T, 6, HIGH, HIGH, generator=g); tgt[:, :, 0] = tgt[:, :, 0] * 2 - 1
    batch = (inp.cuda(), flow.cuda(), tgt.cuda())
    with contextlib.redirect_stdout(sys.stderr):
        torch.manual_seed(0)
        first = models.createNetwork('EnhanceNet', 4, 101, [0, 1, 2, 3, 4], 6, opt)
        criterion = losses.LossNetUnshaded("cuda", 5, 6, HIGH, PAD, opt).to("cuda")
    kinds = {"kernels": True, "torch": False}
    nets, opts, graphs = {}, {}, {}
    for kind, flag in kinds.items():
        ops.BATCH_NORM_KERNELS = flag
        for form in ("eager", "graph"):
            key = (kind, form)
            nets[key] = copy.deepcopy(first).train().cuda()
            opts[key] = train.make_optimizer(nets[key], lr=1e-4, capturable=True)[0]
        graphs[kind] = train.GraphedTrainStep(nets[kind, "graph"], criterion, opts[kind, "graph"], batch, warmup=2, initial_image="zero")
    ops.BATCH_NORM_KERNELS = True

    def eager_step(kind):
        key = (kind, "eager")
        opts[key].zero_grad()
        loss, loss_sum = train.clip_loss(nets[key], criterion, *batch, initial_image="zero")
        train.backward(loss)
        opts[key].step()
        return loss_sum

    def timed(kind, form, steps):
        ops.BATCH_NORM_KERNELS = kinds[kind]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = eager_step(kind) if form == "eager" else graphs[kind](batch)
        torch.cuda.synchronize()
        ops.BATCH_NORM_KERNELS = True
        assert torch.isfinite(loss).all()
        return (time.perf_counter() - t0) / steps * 1e3

    forms = [(kind, form) for form in ("eager", "graph") for kind in kinds]
    for key in forms:
        timed(*key, args.warmup)
    ms = {"%s_%s" % key: [] for key in forms}
    for _ in range(args.rounds):
        for key in forms:
            ms["%s_%s" % key].append(round(timed(*key, args.steps), 3))
    tables = {}
    for kind, flag in kinds.items():
        ops.BATCH_NORM_KERNELS = flag
        ops.profile_enable(True)
        try:
            eager_step(kind)
            torch.cuda.synchronize()
            per = {}
            for name, _, v in ops.profile_records():
                launches, total = per.get(name, (0, 0.0))
                per[name] = (launches + 1, total + v)
        finally:
            ops.profile_enable(False)
            ops.BATCH_NORM_KERNELS = True
        whole = sum(v for _, v in per.values())
        tables[kind] = {"launches_of_this_package": sum(c for c, _ in per.values()), "device_ms_of_this_package": round(whole, 3),
                        "by_kernel": {name: {"launches": c, "ms": round(v, 4), "share_of_package_ms": round(v / whole, 4)}
                                      for name, (c, v) in sorted(per.items(), key=lambda kv: -kv[1][1])}}
    print(json.dumps({"network": "EnhanceNet useBN, 101 -> 6", "clip": [B, T, LOW, HIGH], "steps": args.steps,
                      "ms_per_step": ms, "profiled_eager_step": tables}))


if __name__ == "__main__":
    main()
