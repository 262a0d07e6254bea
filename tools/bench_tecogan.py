"""The TecoGAN generator on the HIP path: its transposed convolution alone, and whole colour frames beside the colour EnhanceNet's.

    python tools/bench_tecogan.py [--reps 60] [--rounds 3] [--steps 20] [--warmup 15] [--skip-frames] [--skip-kernels]

Kernels (per size 270x480 -> 540x960 and 540x960 -> 1080x1920, 64 -> 64 channels, LeakyReLU): device-event times of
  split     ops.conv_transpose3x3_s2 on isrConvTranspose3x3S2ForwardSplit (csrc/sr_conv_transpose.hip),
  torch     F.conv_transpose2d + F.leaky_relu (what the layer ran on before: MIOpen / ATen),
  embedded  the four phases as zero-padded 3x3 taps of a [256, 64, 3, 3] weight on ops.conv3x3_split + F.pixel_shuffle,
  exact     the same on the exact fp32 kernel (the range guard's route),
  fill/copy a write of the output's bytes (tensor.fill_) and a copy of them (tensor.copy_): what the box's memory system gives a
            kernel that only stores / only moves that many bytes,
INTERLEAVED (one of each per repetition), median of --reps repetitions after 10 warm-up repetitions.
Frames: bench_colour.py's loop (ejecta256, 480x270 -> 1920x1080, next frame's ray-march prefetched) for a colour TecoGAN (56 in, 3 out,
10 blocks) and the colour EnhanceNet, interleaved rounds, + the TecoGAN frame's per-kernel milliseconds from the dispatch-packet events.
Prints one JSON line."""
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
    out = {}
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(64, 64, 3, 3, generator=g) * (2.0 / (9 * 64)) ** 0.5).cuda()
    b = (torch.randn(64, generator=g) * 0.05).cuda()
    we, be = ops.conv_transpose_phase_weight(w), b.repeat_interleave(4).contiguous()
    for h, wd in ((270, 480), (540, 960)):
        x = torch.randn(1, 64, h, wd, generator=g).cuda()
        hot = x.clone()
        hot._isr_range_key = ops.HOT
        big = torch.empty(1, 64, 2 * h, 2 * wd, device="cuda")
        src = torch.randn(1, 64, 2 * h, 2 * wd, device="cuda")
        forms = {
            "split": lambda: ops.conv_transpose3x3_s2(x, w, b, act='leaky'),
            "torch": lambda: F.leaky_relu(F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1), 0.01),
            "embedded": lambda: F.pixel_shuffle(ops.conv3x3_split(x, we, be, act='leaky'), 2),
            "exact": lambda: ops.conv_transpose3x3_s2(hot, w, b, act='leaky'),
            "fill": lambda: big.fill_(1.0),
            "copy": lambda: big.copy_(src),
        }
        ms = {k: [] for k in forms}
        with torch.no_grad():
            ref = forms["split"]()
            others = {k: (forms[k]() - ref).abs().max().item() for k in ("torch", "embedded", "exact")}      # the same function
            for rep in range(reps + 10):
                for k, f in forms.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); f(); e1.record()
                    e1.synchronize()
                    if rep >= 10:
                        ms[k].append(e0.elapsed_time(e1))
        nbytes = 64 * 4 * h * wd * 4
        out["%dx%d" % (h, wd)] = {"median_ms": {k: round(statistics.median(v), 4) for k, v in ms.items()},
                                  "min_ms": {k: round(min(v), 4) for k, v in ms.items()},
                                  "output_MB": round(nbytes / 1e6, 1), "GMAC": round(9 * 64 * 64 * h * wd / 1e9, 2),
                                  "max_abs_difference_from_split": others}
    return out


def frame_rates(rounds, steps, warmup):
    from isosurfacesuperresolution_amd import models, ops, volumes as V
    from isosurfacesuperresolution_amd.inference import DirectRenderer, LoadedModel
    from isosurfacesuperresolution_amd.pipeline import SuperResolutionPipeline, default_shading
    renderer = DirectRenderer()
    renderer.load_dense(V.VOLUMES["ejecta256"][0]())
    opt = argparse.Namespace(upsample='bilinear', reconType='residual', useBN=False, numResidualLayers=10)
    origins = [V.orbit_camera(k - warmup, K=max(64, steps)) for k in range(warmup + steps + 1)]
    nets = {}
    with contextlib.redirect_stdout(sys.stderr):
        for name in ("EnhanceNet", "TecoGAN"):
            torch.manual_seed(0)
            nets[name] = models.createNetwork(name, 4, 56, [0, 1, 2], 3, opt)

    def run(kind, profile=False):
        model = LoadedModel.from_model(nets[kind], "cuda", parameters={"initialImage": "zero"})
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
        for k in range(steps):
            pipe.frame(origins[warmup + k], origins[warmup + k + 1])
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        per = {}
        if profile:
            for name, _, ms in ops.profile_records():
                per[name] = per.get(name, 0.0) + ms / steps
            ops.profile_enable(False)
        pipe.close()
        return steps / elapsed, per

    fps = {k: [] for k in nets}
    with torch.no_grad():
        for _ in range(rounds):
            for kind in nets:
                fps[kind].append(round(run(kind)[0], 1))
        kernels = {n: round(v, 4) for n, v in run("TecoGAN", profile=True)[1].items()}
    return {"frames_per_s": fps, "tecogan_kernel_ms_per_frame": kernels}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--skip-frames", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tecogan.py measures on the GPU"
    result = {}
    if not args.skip_kernels:
        result["kernels"] = kernel_times(args.reps)
    if not args.skip_frames:
        result["frames"] = frame_rates(args.rounds, args.steps, args.warmup)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
