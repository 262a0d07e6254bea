"""Colour against unshaded frames at bench.py's default shapes: the 256^3 ejecta volume, 480x270 -> 1920x1080, the next frame's
ray-march prefetched beside the network, 20 timed frames after warm-up -- the same loop for a colour model (RGB + mask + normal + depth
in, RGB out: 56 input channels, three outputs) and for the unshaded model (101 in, six out), INTERLEAVED in one process on one box.

    python tools/bench_colour.py [--rounds 3] [--steps 20] [--warmup 15] [--variant 8] [--only colour|unshaded]

Prints one JSON line: frames/s of every round of both models (the unshaded rounds' spread is the box's run-to-run spread in this
session) and the per-kernel milliseconds per frame of the colour frame from the libraries' dispatch-packet events (a pass of its own,
outside the timed loops).  `--only colour` runs the colour loop alone: the program to put after `--` of
`rocprofv3 --kernel-trace --stats` (profiles/colour_frame.md)."""
import argparse
import contextlib
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--variant", type=int, default=8, choices=[8, 7, 5, 4])
    ap.add_argument("--low", default="480x270")
    ap.add_argument("--volume", default="ejecta256")
    ap.add_argument("--only", default=None, choices=["colour", "unshaded"])
    args = ap.parse_args()
    from isosurfacesuperresolution_amd import models, ops, volumes as V
    from isosurfacesuperresolution_amd.inference import DirectRenderer, LoadedModel
    from isosurfacesuperresolution_amd.pipeline import SuperResolutionPipeline, default_shading
    low_w, low_h = (int(v) for v in args.low.split("x"))
    renderer = DirectRenderer()
    renderer.load_dense(V.VOLUMES[args.volume][0]())
    opt = argparse.Namespace(upsample='bilinear', reconType='residual', useBN=False, numResidualLayers=10)
    K, Wm = args.steps, args.warmup
    origins = [V.orbit_camera(k - Wm, K=max(64, K)) for k in range(Wm + K + 1)]
    nets = {}
    with contextlib.redirect_stdout(sys.stderr):
        torch.manual_seed(0)
        nets["unshaded"] = models.createNetwork('EnhanceNet', 4, 101, [0, 1, 2, 3, 4], 6, opt)
        torch.manual_seed(0)
        nets["colour"] = models.createNetwork('EnhanceNet', 4, args.variant + 48, [0, 1, 2], 3, opt)
    kinds = [args.only] if args.only else ["unshaded", "colour"]

    def run(kind, profile=False):
        # a freshly loaded model per run (the guard words are per model: LoadedModel resets them), as bench.py does per process
        model = LoadedModel.from_model(nets[kind], "cuda", parameters={"initialImage": "zero"})
        pipe = SuperResolutionPipeline(renderer, model, default_shading("cuda", 30.0), (low_w, low_h), graph=False)
        pipe.set_static(fov=30.0, isovalue=0.34)
        for k in range(Wm):
            pipe.frame(origins[k], origins[k + 1])
        torch.cuda.synchronize()
        pipe.reset()
        for k in range(max(0, Wm - 2), Wm):
            pipe.frame(origins[k], origins[k + 1])
        if profile:
            ops.profile_enable(True, small_kernels=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(K):
            pipe.frame(origins[Wm + k], origins[Wm + k + 1])
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        per = {}
        if profile:
            for name, _, ms in ops.profile_records():
                per[name] = per.get(name, 0.0) + ms / K
            ops.profile_enable(False)
        pipe.close()
        return K / elapsed, per

    fps = {k: [] for k in kinds}
    with torch.no_grad():
        for _ in range(args.rounds):
            for kind in kinds:
                fps[kind].append(round(run(kind)[0], 1))
        kernels = {kind: {n: round(v, 4) for n, v in run(kind, profile=True)[1].items()} for kind in kinds}
    print(json.dumps({"workload": "%s, %dx%d -> %dx%d, %d timed frames after %d, next frame prefetched" % (args.volume, low_w, low_h, 4 * low_w, 4 * low_h, K, Wm),
                      "colour_input_channels": args.variant + 48, "frames_per_s": fps, "kernel_ms_per_frame": kernels}))


if __name__ == "__main__":
    main()
