"""What making training clips costs: the generator (``datagen.generate_clips``: frames packed into device-resident clip buffers by one
launch each, nothing read back) against the composition the package had before it (``dataset_video.render_clip``: per-frame torch
assembly on permuted views, host arrays, then ``DeviceClips(DatasetData)`` uploading them again), on one volume, in one process, the two
routes alternating.  The reference's configuration: 512^2 / 128^2 frames, 10 frames per clip, 256 world-space AO rays of radius 1.0.

    python tools/bench_datagen.py [--volume ejecta256] [--clips 2] [--rounds 3] [--semantics gvdb] [--aosamples 256] [--high 512]

Both routes render the same camera paths (the generator's, from one seed; ``render_clip`` takes the origins and keeps its fixed look-at)
with the same isovalue, AO setting and semantics, and end with the clips in ``DeviceClips``' buffers.  A window is one route making
--clips clips, between two device synchronisations; one untimed clip per route comes first.  Then, in a pass of its own with the
per-dispatch timers on (``isoProfile*`` for the ray-marcher, ``isrProfile*`` level 2 for flow fill and pack), ms per frame of the
generator split into ray-march (low, high), flow fill, pack and everything else (wall time minus those).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VOLUMES = {"ejecta256": ("ejecta", 256, (0.30, 0.40)), "ejecta128": ("ejecta", 128, (0.30, 0.40)), "cloud512": ("cloud", 512, (0.25, 0.35)),
           "sphere64": ("sphere64", None, (0.4, 0.6))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volume", choices=sorted(VOLUMES), default="ejecta256")
    ap.add_argument("--clips", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--high", type=int, default=512)
    ap.add_argument("--downscale", type=int, default=4)
    ap.add_argument("--aosamples", type=int, default=256)
    ap.add_argument("--aoradius", type=float, default=1.0)
    ap.add_argument("--semantics", choices=("gvdb", "cpu"), default="gvdb")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    from isosurfacesuperresolution_amd import datagen, dataset_video as D, inference, ops, volumes as V
    assert torch.cuda.is_available(), "bench_datagen.py measures on the GPU"
    name, n, iso_range = VOLUMES[args.volume]
    renderer = inference.DirectRenderer()
    renderer.load_dense(getattr(V, name)(n) if n else getattr(V, name)())
    T, low = args.frames, args.high // args.downscale

    def generator(clips, seed):
        made = datagen.generate_clips(renderer, clips, T, args.high, args.downscale, args.aosamples, args.aoradius, iso_range, seed, "cuda",
                                      args.semantics)
        torch.cuda.synchronize()
        return made

    def composition(clips, seed):
        rng = np.random.RandomState(seed)
        renderer.send_command("semantics", args.semantics)
        highs, lows, flows = [], [], []
        for _ in range(clips):
            p = datagen.random_clip_parameters(rng, *iso_range)
            origins = [[float(v) for v in c[0]] for c in datagen.clip_cameras(p, T)]
            high, low_, flow = D.render_clip(renderer, origins, (low, low), args.downscale, datagen.FOV, p.isovalue, args.aosamples, args.aoradius)
            highs.append(high); lows.append(low_); flows.append(flow)
        r = args.downscale
        sample = D.Sample(0, (0, 32, 0, 32), (0, 32 * r, 0, 32 * r), 0)
        resident = D.DeviceClips(D.DatasetData([sample], highs, lows, flows, 5, 6, 32, T), "cuda")
        torch.cuda.synchronize()
        return resident

    routes = (("generator", generator), ("composition", composition))
    for _, route in routes:                              # warm-up: code objects, workspaces, the allocator's blocks
        route(1, args.seed)
    seconds = {name_: [] for name_, _ in routes}
    for k in range(args.rounds):
        for name_, route in (routes if k % 2 == 0 else routes[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            made = route(args.clips, args.seed + 1 + k)
            seconds[name_].append(time.perf_counter() - t0)
            del made
    # the generator's frame, stage by stage
    renderer.profile_enable(True)
    was = ops.profile_is_on()
    ops.profile_enable(True, small_kernels=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    generator(1, args.seed + 100)
    wall_ms = (time.perf_counter() - t0) * 1e3
    march = renderer.profile_times_ms()
    records = ops.profile_records()
    renderer.profile_enable(False)
    ops.profile_enable(was)
    assert len(march) == 2 * T, (len(march), T)          # low, high, low, high, ...
    fill = sum(ms for kernel, _, ms in records if kernel.startswith("flow_fill"))
    pack = [ms for kernel, _, ms in records if kernel == "clip_pack_kernel"]
    assert len(pack) == T
    stages = {"raymarch_low": sum(march[0::2]) / T, "raymarch_high": sum(march[1::2]) / T, "flow_fill": fill / T, "pack": sum(pack) / T}
    stages["everything_else"] = wall_ms / T - sum(stages.values())
    frame_bytes = 4 * (12 + 6) * args.high ** 2 + 4 * (12 + 5 + 2 + 2) * low ** 2      # what the pack launch reads and writes
    result = {
        "config": {k: getattr(args, k) for k in ("volume", "clips", "rounds", "frames", "high", "downscale", "aosamples", "aoradius", "semantics")},
        "seconds_per_window": seconds,
        "clips_per_second": {k: [args.clips / s for s in v] for k, v in seconds.items()},
        "ms_per_frame": {k: [1e3 * s / (args.clips * T) for s in v] for k, v in seconds.items()},
        "generator_no_slower_in_every_round": all(g <= c for g, c in zip(seconds["generator"], seconds["composition"])),
        "profiled_clip": {"wall_ms_per_frame": wall_ms / T, "stages_ms_per_frame": stages,
                          "pack_GB_per_s": frame_bytes / (1e6 * stages["pack"]) if stages["pack"] > 0 else None},
    }
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
