"""What feeds the captured training step: ms per step of ``train.fit``'s inner loop (batch from the loader, ``.to(device)``, one replay of
``train.GraphedTrainStep``) under three feeds of the SAME clips and samples, one process, one commit, alternating:

    host0   DataLoader(DatasetFromSamples, num_workers=0, shuffle=True)   -- the reference's configuration
    host8   the same with --workers worker processes (default 8)
    device  dataset_video.DeviceBatchLoader(shuffle=True)                 -- clips resident on the GPU, a batch = one gather launch

and, next to them, the floor (the same graph replayed on one resident batch) and the gather launch alone by device events (3 warm-ups,
20 launches) beside a ``copy_`` of the same target tensor device to device.  Network, recipe and batch of ``bench.py --mode train``:
EnhanceNet 101 -> 6, 16 clips x 10 frames, 32^2 -> 128^2, flat Adam.  The clips are generated from a seed at the reference's size
(10 x 6 x 512^2 high, 128^2 low); crops are drawn uniformly (no coverage test: the bytes moved are the same).

    python tools/bench_fit_loader.py [--steps 50] [--warmup 5] [--rounds 2] [--clips 8] [--workers 8]

A window is --steps steps after --warmup steps of the same pass over the loader, between two device synchronisations.  Prints one JSON
line; ``ok`` says that the device feed was no slower than either host feed in every round."""
import argparse
import contextlib
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RECIPE = "l1:mask:1,l1:ao:1,l1:normal:10,l1:depth:10,temp-l2:color:0.1"
B, T, CROP, R, LOW = 16, 10, 32, 4, 128


def make_dataset(D, clips, samples, seed):
    rng = np.random.default_rng(seed)
    highs, lows, flows = [], [], []
    for _ in range(clips):
        low = rng.random((T, 5, LOW, LOW), dtype=np.float32)
        low[:, 0] = low[:, 0] * 2 - 1
        lows.append(low)
        flows.append((rng.random((T, 2, LOW, LOW), dtype=np.float32) - 0.5) * np.float32(0.05))
        high = rng.random((T, 6, R * LOW, R * LOW), dtype=np.float32)
        high[:, 0] = high[:, 0] * 2 - 1
        highs.append(high)
    pick = random.Random(seed)
    table = []
    for _ in range(samples):
        x, y = pick.randint(0, LOW - CROP - 1), pick.randint(0, LOW - CROP - 1)
        table.append(D.Sample(pick.randint(0, clips - 1), (x, x + CROP, y, y + CROP), (R * x, R * (x + CROP), R * y, R * (y + CROP)),
                              pick.randrange(D.MAX_AUGMENTATION_MODE)))
    table.sort(key=lambda s: s.index)
    return D.DatasetData(table, highs, lows, flows, 5, 6, CROP, T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--workers", type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fit_loader.py measures on the GPU"
    from isosurfacesuperresolution_amd import dataset_video as D, losses, models, ops, train
    dev = "cuda"
    per_pass = args.warmup + args.steps
    dd = make_dataset(D, args.clips, B * per_pass, 0)
    resident = D.DeviceClips(dd, dev)
    opt = argparse.Namespace(upsample='bilinear', reconType='residual', useBN=False, numResidualLayers=10, losses=RECIPE,
                             lossAO=0.0, lossAmbient=0.1, lossDiffuse=0.9, lossSpecular=0.0)
    torch.manual_seed(124)
    with contextlib.redirect_stdout(sys.stderr):
        net = models.createNetwork('EnhanceNet', 4, 101, [0, 1, 2, 3, 4], 6, opt).to(dev)
        crit = losses.LossNetUnshaded(dev, 5, 6, R * CROP, CROP // 2, opt).to(dev)
    optim, _ = train.make_optimizer(net, capturable=True, flat=True)
    host_set = D.DatasetFromSamples(dd, False, 0.0)
    feeds = {
        "host0": lambda: torch.utils.data.DataLoader(host_set, batch_size=B, shuffle=True, num_workers=0),
        "host%d" % args.workers: lambda: torch.utils.data.DataLoader(host_set, batch_size=B, shuffle=True, num_workers=args.workers, timeout=300),
        "device": lambda: D.DeviceBatchLoader(resident, B, test_fraction=0.0, shuffle=True, seed=1),
    }
    one = next(iter(feeds["device"]()))
    step = train.GraphedTrainStep(net, crit, optim, one, initial_image="zero")

    def window(loader):
        """fit's inner loop over one pass of ``loader``; the clock runs from the end of step --warmup to the end of the pass."""
        t0, steps, loss = None, 0, None
        for k, batch in enumerate(loader):
            if k == args.warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            batch = tuple(t.to(dev, non_blocking=True) for t in batch)
            loss = step(batch)
            steps += k >= args.warmup
        torch.cuda.synchronize()
        assert steps == args.steps and torch.isfinite(loss).all()
        return (time.perf_counter() - t0) / steps * 1e3

    def floor():
        for _ in range(args.warmup):
            step(one)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step(one)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    ms = {name: [] for name in list(feeds) + ["floor"]}
    for _ in range(args.rounds):
        for name, make in feeds.items():
            ms[name].append(round(window(make()), 3))
        ms["floor"].append(round(floor(), 3))

    # the gather launch alone, and a plain device-to-device copy of the same target tensor
    idx = torch.arange(B, device=dev)
    target = one[2]
    dst = torch.empty_like(target)

    def events(fn, warm=3, n=20):
        for _ in range(warm):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e3
    gather_us = events(lambda: ops.gather_clips(resident, resident.samples, idx, CROP, False))
    gather_aug_us = events(lambda: ops.gather_clips(resident, resident.samples, idx, CROP, True))
    copy_us = events(lambda: dst.copy_(target))
    batch_bytes = sum(t.numel() * 4 for t in one)
    best = {name: min(v) for name, v in ms.items()}
    hosts = [name for name in feeds if name != "device"]
    print(json.dumps({
        "workload": "EnhanceNet training step, %d clips x %d frames, %d^2 -> %d^2, GraphedTrainStep, flat Adam" % (B, T, CROP, R * CROP),
        "clips": args.clips, "resident_bytes": resident.nbytes, "batch_bytes": batch_bytes, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": ms, "device_minus_floor_ms": round(best["device"] - best["floor"], 3),
        "gather_us": round(gather_us, 2), "gather_augmented_us": round(gather_aug_us, 2), "gather_gbytes_per_s": round(2 * batch_bytes / gather_us / 1e3, 1),
        "copy_target_us": round(copy_us, 2), "copy_gbytes_per_s": round(2 * target.numel() * 4 / copy_us / 1e3, 1),
        "gather_over_copy": round(gather_us / copy_us, 3),
        "ok": all(d <= h for name in hosts for d, h in zip(ms["device"], ms[name]))}))


if __name__ == "__main__":
    main()
