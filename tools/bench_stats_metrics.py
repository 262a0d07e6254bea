"""The metric stage of the statistics harness, per frame: ``stats.Statistics.add_timestep_sample`` with ``metrics="torch"`` (fp64
``F.conv2d`` / ``avg_pool2d`` chains, ``.item()`` per column, ``np.histogram`` on the host) against ``metrics="hip"`` (the kernels of
csrc/sr_metrics.hip) on ONE seeded 1920 x 1080 pair (low 480 x 270; border 15: the metrics see 1800 x 960).

Both paths ALTERNATE in one process: after a warm-up of each, every repeat times ``--frames`` calls of one path and then of the other,
each timed region ended by a synchronise.  Prints one JSON line: milliseconds per frame of every repeat of both paths (the torch
path's spread is what the difference has to exceed), and the largest difference between the two paths' rows.

    python tools/bench_stats_metrics.py [--repeats 5] [--frames 3] [--warmup 2] [--only torch|hip]

``--only hip --repeats 1`` under ``rocprofv3 --kernel-trace --stats`` gives the per-kernel times."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def seeded_frame(low_h, low_w, device):
    """(prediction, ground truth, low-resolution input): a shaded blob that covers most of the frame, the prediction a little off."""
    from isosurfacesuperresolution_amd.utils import ScreenSpaceShading
    g = torch.Generator().manual_seed(2024)
    H, W = 4 * low_h, 4 * low_w
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    r2 = (xx ** 2 + yy ** 2) / 0.8
    inside = (r2 < 1.0).float()
    nz = torch.sqrt((1.0 - r2).clamp_min(1e-4))
    n = torch.nn.functional.normalize(torch.stack([xx, yy, nz]), dim=0) * inside
    gt = torch.cat([(inside * 2 - 1).unsqueeze(0), n, ((0.4 + 0.3 * nz) * inside).unsqueeze(0), ((0.6 + 0.4 * nz) * inside + (1 - inside)).unsqueeze(0)])
    gt = (gt + 0.01 * torch.rand(gt.shape, generator=g) * inside).unsqueeze(0)
    pred = gt + 0.03 * (torch.rand(gt.shape, generator=g) - 0.5)
    pred = torch.cat([pred[:, 0:1].clamp(-1, 1), ScreenSpaceShading.normalize(pred[:, 1:4], dim=1), pred[:, 4:6].clamp(0, 1)], dim=1)
    low = torch.nn.functional.avg_pool2d(gt[:, :5], 4)
    return pred.to(device), gt.to(device), low.to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--low", default="480x270")
    ap.add_argument("--only", default=None, choices=("torch", "hip"))
    args = ap.parse_args()
    from isosurfacesuperresolution_amd import stats
    low_w, low_h = (int(v) for v in args.low.split("x"))
    pred, gt, low = seeded_frame(low_h, low_w, "cuda")
    names = [args.only] if args.only else ["torch", "hip"]
    st = {n: stats.Statistics("cuda", metrics=n) for n in names}

    def run(name, frames):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(frames):
            assert st[name].add_timestep_sample(pred, gt, low)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1000.0 / frames
    ms = {n: [] for n in names}
    with torch.no_grad():
        for n in names:
            run(n, args.warmup)
        for _ in range(args.repeats):
            for n in names:
                ms[n].append(round(run(n, args.frames), 3))
    rows = {n: st[n].sample_row() for n in names}
    out = {"workload": "%dx%d -> %dx%d, border %d, %d frames per timed region after %d" % (low_w, low_h, 4 * low_w, 4 * low_h, stats.BORDER,
                                                                                             args.frames, args.warmup),
           "ms_per_frame": ms, "row": {n: [float("%.9g" % v) for v in r] for n, r in rows.items()}}
    if len(names) == 2:
        out["max_abs_row_difference"] = max(abs(a - b) for a, b in zip(rows["torch"], rows["hip"]))
        out["torch_spread_ms"] = round(max(ms["torch"]) - min(ms["torch"]), 3)
        out["speedup_of_medians"] = round(sorted(ms["torch"])[len(ms["torch"]) // 2] / sorted(ms["hip"])[len(ms["hip"]) // 2], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
