"""The RCAN generator on the HIP path: its three non-convolution kernels alone, and whole colour frames of the full 10 x 20 network --
with those three pieces on the kernels of csrc/sr_attention.hip and, for comparison, on PyTorch-ROCm's operators.

    python tools/bench_rcan.py [--reps 60] [--rounds 3] [--steps 20] [--warmup 15] [--skip-frames] [--skip-kernels]

Kernels (64 channels at 270 x 480, the tail 270 x 480 -> 3 x 1080 x 1920): device-event times, INTERLEAVED (one of each per repetition),
median and minimum of --reps repetitions after 10 warm-up repetitions, of
  pool / pool_torch            ops.channel_pool (isrChannelPool + isrChannelPoolMean) / torch.mean
  attention / attention_torch  ops.channel_attention_residual (isrChannelPool + isrChannelGateScaleAdd) / mean, linear, leaky_relu, linear,
                               sigmoid, mul, add
  tail / tail_torch            ops.pixel_shuffle4_conv(clamp=True) (isrShuffleTailColour) / pixel_shuffle, conv2d, clamp
  copy                         tensor.copy_ of one 64 x 270 x 480 tensor: what the box gives a kernel that reads and writes those bytes
and the bytes each new kernel must move (pool: one read of t; gate: x and t read, y written; tail: f read, the frame written).
Frames: bench_colour.py's loop (ejecta256, 480x270 -> 1920x1080, next frame's ray-march prefetched, fused frame path) for a colour RCAN
(56 in, 3 out, 10 groups x 20 blocks, PyTorch's default initialisation), ``ops.ATTENTION_KERNELS`` on and off in interleaved rounds, +
the per-kernel milliseconds of a frame from the dispatch-packet events (kernels of this package only).  Prints one JSON line."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernel_times(reps):
    from isosurfacesuperresolution_amd import ops
    g = torch.Generator().manual_seed(0)
    h, w = 270, 480
    x, t = torch.randn(1, 64, h, w, generator=g).cuda(), torch.randn(1, 64, h, w, generator=g).cuda()
    wd, bd = (torch.randn(4, 64, generator=g) / 8).cuda(), (torch.randn(4, generator=g) * 0.1).cuda()
    wu, bu = (torch.randn(64, 4, generator=g) / 2).cuda(), (torch.randn(64, generator=g) * 0.1).cuda()
    wt, bt = (torch.randn(3, 4, 3, 3, generator=g) * 0.1).cuda(), (torch.randn(3, generator=g) * 0.05 + 0.5).cuda()
    dst = torch.empty_like(x)

    def attention_torch():
        s = torch.sigmoid(F.linear(F.leaky_relu(F.linear(t.mean(dim=(2, 3)), wd, bd), 0.01), wu, bu))
        return x + t * s[:, :, None, None]
    forms = {
        "pool": lambda: ops.channel_pool(t),
        "pool_torch": lambda: t.mean(dim=(2, 3)),
        "attention": lambda: ops.channel_attention_residual(x, t, wd, bd, wu, bu),
        "attention_torch": attention_torch,
        "tail": lambda: ops.pixel_shuffle4_conv(x, wt, bt, clamp=True),
        "tail_torch": lambda: torch.clamp(F.conv2d(F.pixel_shuffle(x, 4), wt, bt, padding=1), 0, 1),
        "copy": lambda: dst.copy_(x),
    }
    ms = {k: [] for k in forms}
    with torch.no_grad():
        same = {"attention": (forms["attention"]() - attention_torch()).abs().max().item(),
                "tail": (forms["tail"]() - forms["tail_torch"]()).abs().max().item()}
        for rep in range(reps + 10):
            for k, f in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); f(); e1.record()
                e1.synchronize()
                if rep >= 10:
                    ms[k].append(e0.elapsed_time(e1))
        # the gate launch alone, from the library's own dispatch-packet events (the op above is pool + gate)
        ops.profile_enable(True)
        for _ in range(reps):
            forms["attention"](); forms["tail"]()
        torch.cuda.synchronize()
        per = {}
        for name, _, v in ops.profile_records():
            per.setdefault(name, []).append(v)
        ops.profile_enable(False)
    plane = 64 * h * w * 4
    moved = {"channel_pool_kernel": plane, "gate_scale_add_kernel": 3 * plane, "shuffle_tail_kernel": plane + 3 * 16 * h * w * 4}
    packet = {n: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "MB": round(moved[n] / 1e6, 1),
                  "TB_per_s_at_median": round(moved[n] / statistics.median(v) / 1e9, 2)} for n, v in per.items() if n in moved}
    return {"median_ms": {k: round(statistics.median(v), 4) for k, v in ms.items()}, "min_ms": {k: round(min(v), 4) for k, v in ms.items()},
            "kernels_by_packet_events": packet, "max_abs_difference_from_torch": same}


def frame_rates(rounds, steps, warmup):
    from isosurfacesuperresolution_amd import models, ops, volumes as V
    from isosurfacesuperresolution_amd.inference import DirectRenderer, LoadedModel
    from isosurfacesuperresolution_amd.pipeline import SuperResolutionPipeline, default_shading
    renderer = DirectRenderer()
    renderer.load_dense(V.VOLUMES["ejecta256"][0]())
    origins = [V.orbit_camera(k - warmup, K=max(64, steps)) for k in range(warmup + steps + 1)]
    with contextlib.redirect_stdout(sys.stderr):
        torch.manual_seed(0)
        net = models.createNetwork('RCAN', 4, 56, [0, 1, 2], 3, None)
    hot = {}

    def run(kernels, profile=False):
        n = min(steps, 4) if profile else steps          # (a profiled frame carries ~1 650 events: few frames are enough)
        ops.ATTENTION_KERNELS = kernels
        try:
            model = LoadedModel.from_model(net, "cuda", parameters={"initialImage": "zero"})
            pipe = SuperResolutionPipeline(renderer, model, default_shading("cuda", 30.0), (480, 270), graph=False)
            assert pipe.fused and pipe.colour
            pipe.set_static(fov=30.0, isovalue=0.34)
            for k in range(warmup):
                pipe.frame(origins[k], origins[k + 1])
            torch.cuda.synchronize()
            if profile:
                ops.profile_enable(True, small_kernels=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(n):
                rgb, _ = pipe.frame(origins[warmup + k], origins[warmup + k + 1])
            torch.cuda.synchronize()
            elapsed = time.perf_counter() - t0
            per = {}
            if profile:
                for name, _, ms in ops.profile_records():
                    launches, total = per.get(name, (0, 0.0))
                    per[name] = (launches + 1, total + ms)
                ops.profile_enable(False)
            hot["kernels" if kernels else "torch"] = bool(ops.any_hot("cuda"))
            assert torch.isfinite(rgb).all()
            pipe.close()
            return n / elapsed, {name: {"launches_per_frame": c / n, "ms_per_frame": round(v / n, 4)} for name, (c, v) in per.items()}
        finally:
            ops.ATTENTION_KERNELS = True

    fps = {"kernels": [], "torch": []}
    with torch.no_grad():
        for _ in range(rounds):
            for kind in ("kernels", "torch"):
                fps[kind].append(round(run(kind == "kernels")[0], 2))
        table = run(True, profile=True)[1]
        table_torch = run(False, profile=True)[1]
    return {"frames_per_s": fps, "kernel_ms_per_frame": table, "kernel_ms_per_frame_torch_pieces": table_torch, "any_layer_hot": hot}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--skip-frames", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rcan.py measures on the GPU"
    result = {}
    if not args.skip_kernels:
        result["kernels"] = kernel_times(args.reps)
    if not args.skip_frames:
        result["frames"] = frame_rates(args.rounds, args.steps, args.warmup)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
