"""The display stage (viewer.DisplayStage) at bench.py's default shapes: the 256^3 ejecta volume, 480x270 -> 1920x1080, the next frame's
ray-march prefetched beside the network, 20 timed frames after warm-up -- INTERLEAVED in one process on one box:

    pipeline            SuperResolutionPipeline.frame alone (what bench.py times)
    stage_smooth        + DisplayStage: colour view, post-smoothing 0.5, 8-bit copy -- one isrDisplayFrame launch
    stage_focus         + a 400-pixel focus window rendered at full resolution with 16 AO samples, blended in the same launch
    stage_focus_no_ao   the same window without ray-cast AO (what the window's render costs without its AO rays)
    torch_smooth        + the composition of stage_smooth as the module-path torch operations (viewer.compose_display)

    python tools/bench_display.py [--rounds 3] [--steps 20] [--warmup 15] [--only NAME]

Prints one JSON line: frames/s of every round of every mode (the pipeline rounds' spread is the box's run-to-run spread in this
session), and `display_launch_us`: the isrDisplayFrame launch alone on tensors of the same size, 200 back-to-back launches between two
events (smooth: colour view + post-smoothing + 8-bit copy; focus: the same with the window blended in).  `--only NAME` runs one mode alone."""
import argparse
import contextlib
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODES = {
    "pipeline": None,
    "stage_smooth": dict(channel="color", post_smoothing=0.5, present_uint8=True),
    "stage_focus": dict(channel="color", post_smoothing=0.5, present_uint8=True, focus="window", focus_ao_samples=16),
    "stage_focus_no_ao": dict(channel="color", post_smoothing=0.5, present_uint8=True, focus="window", focus_ao_samples=0),
    "torch_smooth": dict(channel="color", post_smoothing=0.5, present_uint8=True, fused=False),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--low", default="480x270")
    ap.add_argument("--volume", default="ejecta256")
    ap.add_argument("--window", type=int, default=400, help="half width of the focus window in high-resolution pixels")
    ap.add_argument("--only", default=None, choices=list(MODES))
    args = ap.parse_args()
    from isosurfacesuperresolution_amd import models, viewer, volumes as V
    from isosurfacesuperresolution_amd.inference import DirectRenderer, LoadedModel
    from isosurfacesuperresolution_amd.pipeline import SuperResolutionPipeline, default_shading
    low_w, low_h = (int(v) for v in args.low.split("x"))
    renderer = DirectRenderer()
    renderer.load_dense(V.VOLUMES[args.volume][0]())
    opt = argparse.Namespace(upsample='bilinear', reconType='residual', useBN=False, numResidualLayers=10)
    K, Wm = args.steps, args.warmup
    origins = [V.orbit_camera(k - Wm, K=max(64, K)) for k in range(Wm + K + 1)]
    with contextlib.redirect_stdout(sys.stderr):
        torch.manual_seed(0)
        net = models.createNetwork('EnhanceNet', 4, 101, [0, 1, 2, 3, 4], 6, opt)
    names = [args.only] if args.only else list(MODES)

    def run(name):
        # a freshly loaded model per run (the guard words are per model: LoadedModel resets them), as bench.py does per process
        model = LoadedModel.from_model(net, "cuda", parameters={"initialImage": "zero"})
        pipe = SuperResolutionPipeline(renderer, model, default_shading("cuda", 30.0), (low_w, low_h), graph=False)
        pipe.set_static(fov=30.0, isovalue=0.34)
        driver = pipe
        if MODES[name] is not None:
            kw = dict(MODES[name])
            if kw.get("focus") == "window":
                kw["focus"] = ((2 * low_w, 2 * low_h), args.window, args.window // 4)
            driver = viewer.DisplayStage(pipe, **kw)
        for k in range(Wm):
            driver.frame(origins[k], origins[k + 1])
        torch.cuda.synchronize()
        driver.reset()
        for k in range(max(0, Wm - 2), Wm):
            driver.frame(origins[k], origins[k + 1])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(K):
            driver.frame(origins[Wm + k], origins[Wm + k + 1])
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        pipe.close()
        return K / elapsed

    def launch_us():
        from isosurfacesuperresolution_amd import ops
        H, W = 4 * low_h, 4 * low_w
        g = torch.rand(low_h, low_w, 12, device="cuda")
        rgb, raw, prev = torch.rand(1, 3, H, W, device="cuda"), torch.rand(1, 6, H, W, device="cuda"), torch.rand(1, 3, H, W, device="cuda")
        flow = (torch.rand(1, 2, low_h, low_w, device="cuda") - 0.5) * 0.01
        full = torch.rand(H, W, 12, device="cuda")
        region = viewer.focus_region(H, W, (W // 2, H // 2), args.window, args.window // 4, device="cuda")
        out, out8 = torch.empty_like(rgb), torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
        sh = default_shading("cuda", 30.0)
        res = {}
        for name, kw in (("smooth", {}), ("focus", dict(focus=region, focus_gbuffer=full))):
            call = lambda: ops.display_frame(g, rgb, raw, flow, shading=sh, prev_displayed=prev, post_smoothing=0.5, out=out, out8=out8, **kw)
            for _ in range(20):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                call()
            e1.record()
            torch.cuda.synchronize()
            res[name] = round(e0.elapsed_time(e1) * 1000.0 / 200, 1)
        return res

    fps = {n: [] for n in names}
    with torch.no_grad():
        for _ in range(args.rounds):
            for n in names:
                fps[n].append(round(run(n), 1))
    print(json.dumps({"workload": "%s, %dx%d -> %dx%d, %d timed frames after %d, next frame prefetched" % (args.volume, low_w, low_h, 4 * low_w, 4 * low_h, K, Wm),
                      "focus_window": args.window, "frames_per_s": fps, "display_launch_us": launch_us()}))


if __name__ == "__main__":
    main()
