"""One 480 x 270 -> 1920 x 1080 frame of the network (``pipeline.run_network``: dataflow trunk, upsampling layers, fused tail and
finishing) for a batch-norm EnhanceNet in eval mode -- its batch-norm layers folded into their convolutions, ``ops.fold_batch_norm`` --
beside a plain EnhanceNet.  The two run the same launches on weights of the same shapes, so the expectation is equality; the per-frame
cost the batch-norm net adds is the host's staleness check of its 20 folds.

    python tools/bench_bn_frame.py [--frames 200] [--rounds 5] [--warmup 20]

Timing: wall clock around --frames frames between two device synchronisations (what a frame loop sees, the host side included), the
two networks INTERLEAVED (one block of frames of each per round), every round listed.  Prints one JSON line."""
import argparse
import contextlib
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W = 270, 480


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bn_frame.py measures on the GPU"
    from isosurfacesuperresolution_amd import models, ops
    from isosurfacesuperresolution_amd.inference import LoadedModel
    from isosurfacesuperresolution_amd.pipeline import default_shading, run_network
    loaded = {}
    with contextlib.redirect_stdout(sys.stderr):
        for kind, use_bn in (("plain", False), ("batch_norm", True)):
            torch.manual_seed(0)
            opt = argparse.Namespace(upsample='bilinear', reconType='residual', useBN=use_bn, numResidualLayers=10)
            net = models.createNetwork('EnhanceNet', 4, 101, [0, 1, 2, 3, 4], 6, opt)
            if use_bn:                                     # statistics as a trained net has them, not the identity of a fresh layer
                g = torch.Generator().manual_seed(1)
                with torch.no_grad():
                    for m in net.modules():
                        if isinstance(m, torch.nn.BatchNorm2d):
                            m.running_mean.copy_(0.3 * torch.randn(64, generator=g)); m.running_var.copy_(0.5 + 1.5 * torch.rand(64, generator=g))
                            m.weight.copy_(0.5 + torch.rand(64, generator=g)); m.bias.copy_(0.05 * torch.randn(64, generator=g))
            loaded[kind] = LoadedModel.from_model(net, "cuda")
    shading = default_shading("cuda", 30.0)
    x = ops.empty_planes(1, 101, H, W, "cuda")
    x.copy_(torch.rand(1, 101, H, W, generator=torch.Generator().manual_seed(2)))

    def timed(kind, frames):
        with torch.no_grad():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(frames):
                raw, rgb = run_network(loaded[kind], shading, x)
            torch.cuda.synchronize()
        assert torch.isfinite(raw).all()
        return (time.perf_counter() - t0) / frames * 1e3

    names = {}
    for kind in loaded:
        timed(kind, args.warmup)
        ops.profile_enable(True, small_kernels=True)
        timed(kind, 1)
        names[kind] = [r[0] for r in ops.profile_records()]
        ops.profile_enable(False)
    ms = {kind: [] for kind in loaded}
    for _ in range(args.rounds):
        for kind in loaded:
            ms[kind].append(round(timed(kind, args.frames), 4))
    print(json.dumps({"frame": [H, W, 4 * H, 4 * W], "frames": args.frames, "ms_per_frame": ms, "same_launches": names["plain"] == names["batch_norm"],
                      "launches": names["batch_norm"], "range_guard_hot": bool(ops.any_hot("cuda"))}))


if __name__ == "__main__":
    main()
