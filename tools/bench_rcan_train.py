"""Training a full RCAN (10 groups x 20 blocks, 56 in, 3 out) on the HIP path: one optimisation step of a colour clip through
``train.colour_clip_loss`` -- B = 2 clips of T = 3 frames, 32 x 32 -> 128 x 128 crops, L1 + 0.1 temporal MSE as criterion, flat Adam --
eager (``train.train_step``'s sequence) and captured in a HIP graph (``train.GraphedTrainStep``), with the channel attention and the
pixel-shuffle tail on the kernels of csrc/sr_attention.hip (``ops.ATTENTION_KERNELS = True``) and, for comparison, on the torch
composite (``False``; the convolutions run on the HIP training kernels either way).

    python tools/bench_rcan_train.py [--steps 10] [--rounds 3] [--warmup 3] [--groups 10] [--blocks 20]

Timing: wall clock around --steps steps between two device synchronisations, the four forms INTERLEAVED (one block of steps of each
per round), every round listed.  Launches: one eager step under ``ops.profile_enable`` -- the dispatches of THIS PACKAGE's kernels
per step and their device milliseconds by kernel name (``ops.profile_records()``; PyTorch's own launches, which is what the composite
consists of, are not in those records: the composite's column shows what is left on the package's kernels).  Prints one JSON line."""
import argparse
import contextlib
import copy
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, T, LOW, HIGH = 2, 3, 32, 128


def criterion(target, prediction, input_low, previous_warped):
    return (prediction - target).abs().mean() + 0.1 * ((prediction - previous_warped) ** 2).mean(), {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--groups", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rcan_train.py measures on the GPU"
    from isosurfacesuperresolution_amd import models, ops, train
    g = torch.Generator().manual_seed(0)
    batch = (torch.rand(B, T, 8, LOW, LOW, generator=g).cuda(), ((torch.rand(B, T, 2, LOW, LOW, generator=g) - 0.5) * 0.05).cuda(),
             torch.rand(B, T, 3, HIGH, HIGH, generator=g).cuda())
    with contextlib.redirect_stdout(sys.stderr):
        torch.manual_seed(0)
        first = models.createNetwork('RCAN', 4, 56, [0, 1, 2], 3, argparse.Namespace(rcanGroups=args.groups, rcanBlocks=args.blocks))
    kinds = {"kernels": True, "composite": False}
    nets, opts, graphs = {}, {}, {}
    for kind, flag in kinds.items():
        ops.ATTENTION_KERNELS = flag
        for form in ("eager", "graph"):
            key = (kind, form)
            nets[key] = copy.deepcopy(first).train().cuda()
            opts[key] = train.make_optimizer(nets[key], lr=1e-4, capturable=True, flat=True)[0]
        graphs[kind] = train.GraphedTrainStep(nets[kind, "graph"], criterion, opts[kind, "graph"], batch, warmup=2,
                                              clip_loss=train.colour_clip_loss)
    ops.ATTENTION_KERNELS = True

    def eager_step(kind):
        key = (kind, "eager")
        opts[key].zero_grad()
        loss, loss_sum = train.colour_clip_loss(nets[key], criterion, *batch)
        train.backward(loss)
        opts[key].step()
        return loss_sum

    def timed(kind, form, steps):
        ops.ATTENTION_KERNELS = kinds[kind]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = eager_step(kind) if form == "eager" else graphs[kind](batch)
        torch.cuda.synchronize()
        ops.ATTENTION_KERNELS = True
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
        ops.ATTENTION_KERNELS = flag
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
            ops.ATTENTION_KERNELS = True
        whole = sum(v for _, v in per.values())
        tables[kind] = {"launches_of_this_package": sum(c for c, _ in per.values()), "device_ms_of_this_package": round(whole, 3),
                        "by_kernel": {name: {"launches": c, "ms": round(v, 4), "share_of_package_ms": round(v / whole, 4)}
                                      for name, (c, v) in sorted(per.items(), key=lambda kv: -kv[1][1])}}
    print(json.dumps({"network": "RCAN %d x %d, 56 -> 3" % (args.groups, args.blocks), "clip": [B, T, LOW, HIGH], "steps": args.steps,
                      "ms_per_step": ms, "profiled_eager_step": tables}))


if __name__ == "__main__":
    main()
