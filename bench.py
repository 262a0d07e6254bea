#!/usr/bin/env python
"""Headline benchmark: frames/s of (ray-march low-res G-buffer + 4x EnhanceNet SR + screen-space
shading) at a 256^3 volume, 480x270 -> 1920x1080 (BASELINE.json configs[1]).

    python bench.py --gpus N --steps K --warmup W

A "step" is one frame of the orbit camera path of SURVEY.md 8(d) on synthetic data (V256-ejecta
stand-in volume, seeded random-init EnhanceNet weights).  With N > 1 there is one rank per GPU: either
torch.distributed.run launched them (WORLD_SIZE is set), or this process starts them itself
(``launch_ranks``: N fresh children before anything touches a GPU) -- every rank renders its own
contiguous chunk of the sequence, started with ``initialImage``: weak scaling, no
data-path collective.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the line with the timed region's own figures.  ``--full`` adds the
passes and legs after the timed region (per-kernel passes, sequence_start, sustained, exact_f32, f16_fast_mode, cpu_baseline and
parity).  ``--dump-outputs DIR`` writes what the last timed step computed as DIR/<name>.npy (``dump_outputs``).

Two further modes time the collectives SURVEY.md 8(e) defines (each prints its own JSON line, with its own metric):

    --mode train   BASELINE config #3: the mainVideoUnshaded.py step (B=16 clips x T=10 frames, 32^2 -> 128^2 crops, l1 +
                   temp-l2 losses, Adam), the global batch split over the ranks, ONE flat 3.64 MB gradient all-reduce per
                   step captured with the step in a HIP graph (train.DataParallelTrainer.graphed)
    --mode tiled   BASELINE config #5: a 1024^3 volume generated tile-wise, one object-space tile per rank, every rank
                   ray-marches the full 960x540 image, all-gather + nearest-hit composite, 4x SR in screen strips with a
                   second all-gather -> 3840x2160
"""
import argparse
import contextlib
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SPLIT_KERNEL_PREFIXES = ("conv3x3_split", "conv3x3_wgrad_split", "resblock_split", "trunk_dataflow", "trunk_mt")      # three fp16 MFMAs per product


def tally_kernels(records):
    """[(kernel name, algorithmic flops, ms)] of ops.profile_records() -> {name: [flops, seconds, launches]}."""
    out = {}
    for name, flops, ms, *weight in records:          # (an optional 4th element: the record stands for that many launches)
        w = weight[0] if weight else 1
        d = out.setdefault(name, [0.0, 0.0, 0])
        d[0] += flops * w
        d[1] += ms * 1e-3 * w
        d[2] += w
    return out


# kernels the frame pipeline runs on the RENDER stream, beside the network (not part of the main stream's serial chain)
SIDE_STREAM_KERNELS = ("flow_fill_one_kernel",)


def gap_accounting(ms_per_step, per, K, host_ms):
    """Where a frame's time is when it is not inside a kernel of the main stream.  ``per``: tally_kernels() of the timed region;
    ``host_ms``: per-frame host time of the K ``pipe.frame`` calls (enqueue only: nothing in a frame synchronises).
    gap = ms_per_step - sum of the main-stream kernels' own durations: launch gaps, waits on the side stream's events, the
    host falling behind.  A slow run explains itself from this one record: kernel rows unchanged + a large gap = the time is
    BETWEEN kernels; host_enqueue close to ms_per_step = the host was the bottleneck."""
    main = sum(v[1] for n, v in per.items() if n not in SIDE_STREAM_KERNELS and n != "unprofiled") / K * 1e3
    side = sum(v[1] for n, v in per.items() if n in SIDE_STREAM_KERNELS) / K * 1e3
    host = sorted(host_ms)
    return {"main_stream_kernels_ms_per_frame": main, "gap_ms_per_frame": ms_per_step - main,
            "side_stream_kernels_ms_per_frame": side,
            "host_enqueue_ms_per_frame": sum(host) / max(1, len(host)), "host_enqueue_ms_max": host[-1] if host else None,
            "host_enqueue_ms_median": host[len(host) // 2] if host else None,
            "note": "gap = ms_per_step - (sum of main-stream kernel durations from the dispatch-packet events); the ray-march of frame t+1 "
                    "and its flow fill run on the render stream and are not in the sum; host_enqueue = wall time of the pipe.frame() calls"}


def is_split_kernel(name):
    """Kernel families of libisr_sr.so that compute each fp32 product as three fp16 MFMAs on split operands: their MFMA
    ceiling is a third of the dense fp16 peak; every other profiled convolution runs on fp32 MFMA."""
    return name.startswith(SPLIT_KERNEL_PREFIXES)


MFMA_F32_PEAK_TFLOPS = 157.3      # /opt/skills/guides/MI355X_MICROARCH.md, chip-level parameters
MFMA_F16_PEAK_TFLOPS = 2500.0     # dense fp16/bf16 MFMA (same table)
HBM_PEAK_GBS = 8000.0
PMC_TRAFFIC_FILES = ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json", "r01_pmc_traffic.json")   # committed rocprofv3 --pmc passes of this command


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mode", default="infer", choices=["infer", "train", "tiled"])
    ap.add_argument("--volume", default="ejecta256", choices=["ejecta256", "ejecta128", "sphere64"])
    ap.add_argument("--low", default="", help="low-resolution image, WxH (default 480x270; 960x540 in --mode tiled)")
    ap.add_argument("--train-batch", type=int, default=16, help="--mode train: GLOBAL batch (clips), split over the ranks")
    ap.add_argument("--train-frames", type=int, default=10)
    ap.add_argument("--train-crop", type=int, default=32)
    ap.add_argument("--tiled-n", type=int, default=1024, help="--mode tiled: edge of the volume")
    ap.add_argument("--no-temporal", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--raymarch-variant", type=int, default=0)
    ap.add_argument("--side-variant", type=int, default=-1, help="kernel variant of the render that runs under the network (diagnostics)")
    ap.add_argument("--no-fast-mode", action="store_true", help="skip the separately reported fp16 fast-mode leg")
    ap.add_argument("--sustained-frames", type=int, default=2000, help="frames of the `sustained` leg that follows the timed region (0: skip); "
                                                                         "same pipeline, outside `value`")
    ap.add_argument("--no-exact-leg", action="store_true", help="skip the separately reported IEEE-fp32 (exact fmaf-chain kernels) leg")
    ap.add_argument("--exact", action="store_true", help="convolutions on the exact k-ordered fp32 fmaf-chain kernels (fp32 MFMA) instead "
                    "of the split-operand kernels (three fp16 MFMAs per product, fp32-equivalent accuracy)")
    ap.add_argument("--raymarch-large", default="", help="extra leg: the ray-march kernel alone on a volume that exceeds the caches, "
                    "e.g. cloud512@1920x1080 (algorithmic bytes counted by the CPU restatement like the cpu_baseline leg)")
    ap.add_argument("--no-overlap", action="store_true", help="render frame t and super-resolve it back to back on one stream")
    ap.add_argument("--cpu-frames", type=int, default=6, help="frames in the CPU baseline sample (about 2 s each on 16 cores)")
    ap.add_argument("--side-waves", type=int, default=0, help="wave cap of the overlapped ray-march (0 = 4 per CU)")
    ap.add_argument("--graph", action="store_true", help="steady-state frames replay as one HIP graph each (pipeline.py); the per-kernel "
                    "durations of `roofline` / `kernels` then come from an eager pass of the same frames AFTER the timed region "
                    "(a replayed graph has no per-dispatch events)")
    ap.add_argument("--full", action="store_true", help="default mode: after the timed region also run the legs the headline does not need -- "
                    "the per-kernel passes (`kernels` complete, `frame_time`, the ray-march alone), sequence_start, sustained, the exact-fp32 "
                    "and fp16 legs, the CPU baseline with its parity passes.  Without it the line is the timed region's own figures")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="write what the timed path computed in its last step as DIR/<name>.npy "
                    "(float32, or float64 where the value is float64), at most %d MB in all: larger outputs are cut to a fixed seeded "
                    "sample of their elements" % (DUMP_BUDGET_BYTES // 10**6))
    return ap.parse_args(argv)


DUMP_BUDGET_BYTES = 60 * 10**6
DUMP_SEED = 0


def dump_outputs(directory, arrays):
    """Write ``{name: tensor or array}`` as ``directory/<name>.npy`` (float64 stays float64, everything else becomes float32).  The
    arrays are taken smallest first; one that does not fit its even share of what is left of DUMP_BUDGET_BYTES is written as a sample
    of its flattened elements: sorted indices drawn without replacement by numpy's generator seeded with DUMP_SEED, so that two runs
    of the same command -- and two builds -- write the same elements.  Returns {name: description} (printed to stderr)."""
    import numpy as np
    os.makedirs(directory, exist_ok=True)
    host = {}
    for name, a in arrays.items():
        a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
        host[name] = np.ascontiguousarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32)
    left, written = DUMP_BUDGET_BYTES, {}
    for i, (name, a) in enumerate(sorted(host.items(), key=lambda kv: kv[1].nbytes)):
        share = left // (len(host) - i)
        if a.nbytes <= share:
            out, written[name] = a, "whole, shape %s" % (list(a.shape),)
        else:
            k = share // a.itemsize
            idx = np.sort(np.random.default_rng(DUMP_SEED).choice(a.size, size=k, replace=False))
            out, written[name] = a.reshape(-1)[idx], "%d of the %d elements of shape %s (flattened, seed %d)" % (k, a.size, list(a.shape), DUMP_SEED)
        np.save(os.path.join(directory, name + ".npy"), out)
        left -= out.nbytes
    return written


class Job:
    """The process group of one bench run: one process per GPU, RCCL (backend "nccl") unless
    BENCH_DIST_BACKEND=gloo rehearses the multi-rank path (with BENCH_SHARE_DEVICE=1 on a one-GPU box, with
    BENCH_DEVICE=cpu on CPU tensors -- the CPU tests of the train / tiled modes).  A failed init raises: nothing here
    re-executes a process that has touched the GPU."""

    def __init__(self, args):
        import torch
        import torch.distributed as dist
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if self.world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        self.backend = os.environ.get("BENCH_DIST_BACKEND", "nccl")
        self.cpu = os.environ.get("BENCH_DEVICE") == "cpu"
        if self.cpu:
            assert self.backend == "gloo" or self.world == 1, "BENCH_DEVICE=cpu needs BENCH_DIST_BACKEND=gloo"
            self.device = "cpu"
        else:
            assert torch.cuda.is_available(), "bench.py needs an MI355X"
            if os.environ.get("BENCH_SHARE_DEVICE") == "1":
                local_rank = 0
            torch.cuda.set_device(local_rank)
            self.device = "cuda"
        # ranks sharing ONE device (a rehearsal): the all-resident spin kernels (dataflow trunk, one-launch flow fill) need every
        # workgroup of a launch resident at once -- two processes' grids interleaved on the CUs would wait for each other until the
        # 50 ms deadline.  The hint switches those forms off in EVERY mode (ops.set_device_shared)
        self.shared = os.environ.get("BENCH_SHARE_DEVICE") == "1"
        if self.shared and not self.cpu:
            from isosurfacesuperresolution_amd import ops
            ops.set_device_shared(True)
        self.timeout_s = float(os.environ.get("BENCH_DIST_TIMEOUT_S", "120"))
        if self.world > 1:
            # A rank that never arrives (or an RCCL bootstrap that is stuck) must end THIS process with a message and a non-zero
            # exit code well inside the driver's limit -- torch's default is 600 s, which is that limit.  Two phases are bounded
            # and named: the rendezvous (init_process_group) and the first collective (where RCCL builds its rings).
            from datetime import timedelta
            self._phase("init_process_group", lambda: dist.init_process_group(
                "nccl", device_id=torch.device("cuda", local_rank), timeout=timedelta(seconds=self.timeout_s))
                if self.backend == "nccl" else dist.init_process_group(self.backend, timeout=timedelta(seconds=self.timeout_s)))
        assert args.gpus == self.world, "--gpus must equal the number of launched ranks"
        # tensors a collective can take: device tensors with RCCL, CPU tensors with gloo
        self.coll_device = "cuda" if (self.backend == "nccl" and not self.cpu) else "cpu"
        if self.world > 1:
            def first():
                ones = torch.ones(1, dtype=torch.float32, device=self.coll_device)
                dist.all_reduce(ones)
                if not self.cpu:
                    torch.cuda.synchronize()
                assert int(ones.item()) == self.world, "first all-reduce joined %d of %d ranks" % (int(ones.item()), self.world)
            self._phase("first collective (all-reduce)", first)
            # the start-up is bounded; the RUN's collectives get torch's usual limit back (a 1024^3 tile takes a rank tens of seconds
            # to generate while its peers already wait in the next all-reduce)
            try:
                from datetime import timedelta
                from torch.distributed import distributed_c10d as c10d
                c10d._set_pg_timeout(timedelta(seconds=float(os.environ.get("BENCH_DIST_RUN_TIMEOUT_S", "600"))))
            except Exception:      # noqa: BLE001 -- a torch without that hook keeps the start-up limit
                pass

    def _phase(self, name, fn):
        """Run one start-up phase under a deadline of ``timeout_s`` (+ a margin for the backend's own timeout to fire first).  On a
        timeout or an error: one line on stderr naming rank and phase, exit code 3 -- a fresh exit of this process, nothing is
        re-executed.  (The watchdog thread is what ends a phase the backend itself never returns from: an RCCL bootstrap that
        hangs inside a C call cannot be interrupted from Python.)"""
        import threading
        t0 = time.perf_counter()

        def expire():
            sys.stderr.write("bench.py: rank %d/%d: phase '%s' did not finish within %.0f s (MASTER %s:%s, backend %s); exiting 3\n" % (
                self.rank, self.world, name, time.perf_counter() - t0, os.environ.get("MASTER_ADDR"), os.environ.get("MASTER_PORT"), self.backend))
            sys.stderr.flush()
            os._exit(3)
        dog = threading.Timer(self.timeout_s + 15.0, expire)
        dog.daemon = True
        dog.start()
        try:
            fn()
        except BaseException as exc:      # noqa: BLE001 -- whatever the backend raised (DistStoreError, RuntimeError, timeout)
            dog.cancel()
            sys.stderr.write("bench.py: rank %d/%d: phase '%s' failed after %.0f s: %s: %s; exiting 3\n" % (
                self.rank, self.world, name, time.perf_counter() - t0, type(exc).__name__, (str(exc).splitlines() or [""])[0][:300]))
            sys.stderr.flush()
            os._exit(3)
        dog.cancel()

    def sync(self):
        import torch
        import torch.distributed as dist
        if not self.cpu:
            torch.cuda.synchronize()
        if self.world > 1:
            dist.barrier()
            if not self.cpu:
                torch.cuda.synchronize()

    def max_over_ranks(self, value):
        import torch
        import torch.distributed as dist
        if self.world == 1:
            return value
        t = torch.tensor([value], dtype=torch.float64, device=self.coll_device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return t.item()

    def joined_ranks(self):
        """How many ranks the collective backend really joined: a sum of ones over an all-reduce (on DEVICE tensors,
        i.e. through RCCL, when the backend is nccl)."""
        import torch
        import torch.distributed as dist
        if self.world == 1:
            return None
        ones = torch.ones(1, dtype=torch.float32, device=self.coll_device)
        dist.all_reduce(ones)
        return int(ones.item())

    def rank_keys(self):
        """{"backend", "ranks_joined", "rccl_ranks"} of the JSON line: ``rccl_ranks`` says how many ranks RCCL joined and
        is null whenever the collectives went through anything else (a gloo rehearsal must not read as an RCCL run)."""
        n = self.joined_ranks()
        name = None if self.world == 1 else ("rccl" if self.backend == "nccl" else self.backend)
        return {"backend": name, "ranks_joined": n, "rccl_ranks": n if self.backend == "nccl" else None}

    def close(self):
        import torch.distributed as dist
        if self.world > 1:
            dist.destroy_process_group()


def launch_ranks(args, argv):
    """``python bench.py --gpus N`` WITHOUT a launcher (no WORLD_SIZE in the environment): this process becomes the launcher.
    It starts N fresh child processes of the same script and arguments -- one rank per GPU, RANK / LOCAL_RANK / WORLD_SIZE /
    MASTER_ADDR / MASTER_PORT set the way torch.distributed.run sets them -- relays rank 0's stdout (the ONE JSON line),
    sends the other ranks' stdout to stderr, and returns the first non-zero exit code (ending the remaining ranks by their
    exact PIDs when one fails, so that a dead rank cannot leave the others in a collective forever).  The launcher never
    imports torch and never touches a GPU; the children are ordinary processes, nothing is exec'd over an initialised
    runtime.  Under torch.distributed.run (WORLD_SIZE set) this function is not reached."""
    import socket
    import subprocess
    import threading
    n = args.gpus
    port = os.environ.get("MASTER_PORT")
    if not port:
        with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
            s.bind(("127.0.0.1", 0))
            port = str(s.getsockname()[1])
    script = os.path.abspath(sys.argv[0])
    children = []
    for rank in range(n):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR=os.environ.get("MASTER_ADDR", "127.0.0.1"), MASTER_PORT=port)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or n) // n)))
        children.append(subprocess.Popen([sys.executable, script] + list(argv), env=env,
                                         stdout=None if rank == 0 else subprocess.PIPE, stderr=None))

    def to_stderr(rank, pipe):
        for line in iter(pipe.readline, b""):
            sys.stderr.write("[rank %d] %s" % (rank, line.decode(errors="replace")))
        pipe.close()
    relays = [threading.Thread(target=to_stderr, args=(r, c.stdout), daemon=True) for r, c in enumerate(children) if r > 0]
    for t in relays:
        t.start()
    code = 0
    live = set(range(n))
    while live:
        for r in sorted(live):
            rc = children[r].poll()
            if rc is None:
                continue
            live.discard(r)
            if rc != 0 and code == 0:
                code = rc if rc > 0 else 1
                sys.stderr.write("bench.py launcher: rank %d exited with %d; ending the other ranks\n" % (r, rc))
                deadline = time.time() + 20.0          # the others may be on their way out with the same error
                while time.time() < deadline and any(children[o].poll() is None for o in live):
                    time.sleep(0.2)
                for o in live:
                    if children[o].poll() is None:
                        children[o].terminate()
                for o in live:
                    try:
                        children[o].wait(timeout=15)
                    except subprocess.TimeoutExpired:
                        children[o].kill()
        time.sleep(0.05)
    for t in relays:
        t.join(timeout=5)
    return code


def main(argv=None, **hooks):
    args = parse(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        code = launch_ranks(args, sys.argv[1:] if argv is None else argv)
        if code != 0:
            sys.exit(code)
        return None
    job = Job(args)
    try:
        if args.mode == "train":
            result = run_train(args, job)
        elif args.mode == "tiled":
            result = run_tiled(args, job, **hooks)
        else:
            result = run_infer(args, job)
        if job.rank == 0:
            print(json.dumps(result), flush=True)
    finally:
        job.close()
    return result


def run_infer(args, job):
    import numpy as np
    import torch
    import torch.distributed as dist
    from isosurfacesuperresolution_amd import models, ops, volumes as V
    from isosurfacesuperresolution_amd.inference import DirectRenderer, LoadedModel
    from isosurfacesuperresolution_amd.pipeline import SuperResolutionPipeline, default_shading
    assert not job.cpu, "--mode infer measures the HIP path: it needs an MI355X"
    world, rank, backend = job.world, job.rank, job.backend

    if args.exact:
        ops.SPLIT_F16 = False
    low_w, low_h = (int(v) for v in (args.low or "480x270").split("x"))
    iso = {"ejecta256": 0.34, "ejecta128": 0.34, "sphere64": 0.5}[args.volume]
    vol = V.VOLUMES[args.volume][0]()
    renderer = DirectRenderer()
    renderer.load_dense(vol)
    opt = argparse.Namespace(upsample='bilinear', reconType='residual', useBN=False, numResidualLayers=10)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(sys.stderr):      # createNetwork prints its configuration like the reference does
        net = models.createNetwork('EnhanceNet', 4, 101, [0, 1, 2, 3, 4], 6, opt)
    model = LoadedModel.from_model(net, "cuda", parameters={"initialImage": "zero"})
    pipe = SuperResolutionPipeline(renderer, model, default_shading("cuda", 30.0), (low_w, low_h),
                                   temporal=not args.no_temporal, graph=True if args.graph else None)
    pipe.set_static(fov=30.0, isovalue=iso)
    pipe.foreground_variant = args.raymarch_variant
    renderer.set_kernel_variant(args.raymarch_variant)
    overlap = not args.no_overlap
    if args.side_variant >= 0:
        pipe.side_variant = args.side_variant
    if args.side_waves > 0:
        pipe.side_waves = args.side_waves

    K, Wm = args.steps, args.warmup
    first = rank * K                      # this rank's contiguous chunk of the orbit
    origins = [V.orbit_camera(first + k - Wm, K=max(64, world * K)) for k in range(Wm + K + 1)]

    sync = job.sync

    for k in range(Wm):
        pipe.frame(origins[k], origins[k + 1] if overlap else None)
    graph_prewarm = 0
    if pipe.graph and Wm > 0 and overlap:
        # --graph: a captured frame's FIRST replay uploads its executable graph (20-30 ms on the host with the GPU idle, seen in two
        # of six runs when the second slot's first replay fell into the timed region: W = 5 is frame 0 eager, 1 eager, two
        # captures, ONE replay).  The warm-up is extended, untimed, until both slots have replayed twice; reported in the line.
        while pipe.graph_replays < 4 and graph_prewarm < 12:
            k = graph_prewarm % max(1, Wm - 1)
            pipe.frame(origins[k], origins[k + 1])
            graph_prewarm += 1
    torch.cuda.synchronize()
    pipe.reset()
    # The timed region is K frames of a RUNNING sequence (what `sustained` runs for 2 000 frames, what a viewer does): the last
    # `lead` warm-up frames are shown once more after the reset, untimed, so that the first timed frame finds its G-buffer rendered
    # ahead like every later one; the start of a sequence (in-line ray-march, first-frame range check with its host wait) is
    # reported as `sequence_start` (1.86 ms against 1.75 ms for a running frame: it never weighed much in the window).
    # Every timed frame does a whole step: SR of frame t with the ray-march of frame t + 1 beside it, K of each.
    lead = min(Wm, 2)
    for k in range(Wm - lead, Wm):
        pipe.frame(origins[k], origins[k + 1] if overlap else None)
    # Per-kernel durations come from start/stop events carried on the dispatch packets themselves
    # (hipExtLaunchKernelGGL inside the libraries, on the stream the kernels run on): unlike
    # hipEventRecord they add no barrier packets / cache flushes to the timed stream.
    prof_timed = os.environ.get("BENCH_PROFILE_TIMED", "1") != "0" and not pipe.graph
    # the timed region carries events on the CONVOLUTION dispatches only (as every round did); the frame's small kernels are timed
    # in a pass of their own afterwards (BENCH_PROFILE_SMALL=1: inside the timed region too -- an experiment)
    prof_small_timed = os.environ.get("BENCH_PROFILE_SMALL", "0") == "1"
    ops.profile_enable(prof_timed, small_kernels=prof_small_timed)
    renderer.profile_enable(prof_timed)
    replays0 = pipe.graph_replays
    sync()
    host_ms = []
    t0 = time.perf_counter()
    th = t0
    for k in range(K):
        # the next frame's ray-march is enqueued on a side stream and overlaps this frame's network
        rgb, raw = pipe.frame(origins[Wm + k], origins[Wm + k + 1] if overlap else None)
        tn = time.perf_counter()
        host_ms.append((tn - th) * 1e3)
        th = tn
    sync()
    elapsed = time.perf_counter() - t0
    graph_replays = pipe.graph_replays - replays0
    if args.dump_outputs and rank == 0 and K > 0:
        # the last timed frame, before any later pass reuses the pipeline's output buffers
        sys.stderr.write("bench.py: --dump-outputs %s\n" % json.dumps(dump_outputs(args.dump_outputs, {"rgb": rgb, "raw": raw})))
    if pipe.graph and args.full:
        # the per-kernel pass: the same K frames launched eagerly with the dispatch-packet events on (outside the timed region)
        pipe.graph = False
        pipe.reset()
        ops.profile_enable(True, small_kernels=True)
        renderer.profile_enable(True)
        for k in range(K):
            pipe.frame(origins[Wm + k], origins[Wm + k + 1] if overlap and k + 1 < K else None)
        sync()
        pipe.graph = True
    records = ops.profile_records()
    if prof_timed and not prof_small_timed and args.full:
        # the small kernels' durations: the same frames once more, eagerly, outside the timed region
        n_small = min(K, 10)
        pipe.reset()
        ops.profile_enable(True, small_kernels=True)
        for k in range(n_small):
            pipe.frame(origins[Wm + k], origins[Wm + k + 1] if overlap and k + 1 < n_small else None)
        sync()
        scale = K / float(n_small)
        records += [(n, f, ms, scale) for n, f, ms in ops.profile_records() if f == 0.0]      # weighted to the K frames `per` is normalised by
        ops.profile_enable(prof_timed)
    ops.trunk_check()                     # no dataflow launch of the timed region gave up on a neighbour (the error word is sticky)
    switches = ops.debug_switches()
    # an ablation (MFMAs skipped, stores skipped, stamp buffers) must never be behind a reported number; a forced kernel form
    # (ISR_SPLIT_ALGO, an experiment switch) is allowed and shows up in the line
    if os.environ.get("BENCH_ALLOW_SWITCHES") != "1" and os.environ.get("ISR_SR_DIAG") != "1":      # (tools/ab_bench.sh compares kernel forms; the line carries `debug_switches` either way)
        assert not (switches & ~2), "diagnostic switches of libisr_sr.so are set (mask %#x): not a measurement" % switches
    rm_ms = renderer.profile_times_ms()
    ops.profile_enable(False)
    renderer.profile_enable(False)
    elapsed = job.max_over_ranks(elapsed)
    rank_keys = job.rank_keys()

    per = tally_kernels(records)
    if not per:          # BENCH_PROFILE_TIMED=0 (experiment: what the dispatch-packet events cost the timed region)
        per = {"unprofiled": [0.0, 1.0, 1]}
    dominant = max(((n, v) for n, v in per.items() if v[0] > 0 or n == "unprofiled"), key=lambda kv: kv[1][1])      # among the kernels that do matrix work
    dom_name, (dom_flops, dom_time, dom_launches) = dominant
    achieved = dom_flops / dom_time / 1e12
    rm_time = sum(rm_ms) * 1e-3 / max(1, len(rm_ms))
    # the ray-marcher on its own (outside the timed region): the kernel's own figure, next to the one it has as a
    # one-wave-per-SIMD guest under the network
    rm_alone = None if overlap else rm_time
    if overlap and args.full:
        gb = torch.empty((low_h, low_w, 12), dtype=torch.float32, device="cuda")
        renderer.set_kernel_variant(args.raymarch_variant)
        renderer.profile_enable(True)
        for k in range(6):
            renderer.send_command("cameraOrigin", V.fmt3(origins[Wm + (k % K)]))
            renderer.render_async(gb, torch.cuda.current_stream())
        torch.cuda.synchronize()
        alone = renderer.profile_times_ms()[1:]
        renderer.profile_enable(False)
        rm_alone = sum(alone) * 1e-3 / max(1, len(alone))

    # HBM traffic of the dominant kernel: PMC counters cannot be read from inside this process; the
    # committed rocprofv3 --pmc passes of this same command (profiles/r01_pmc_summary.md) provide it.
    traffic = traffic_file = None
    for name in PMC_TRAFFIC_FILES:
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                table = json.load(f)
            key = dom_name if dom_name in table else next(k for k in table if k.startswith(dom_name + "<"))    # template arguments
            traffic = table[key]["traffic_bytes_per_launch"]
            traffic_file = name
            break
        except (OSError, KeyError, ValueError, StopIteration):
            continue
    # Roofline of the dominant kernel.  `achieved` is always ALGORITHMIC: 2*9*Cin*Cout flops per output pixel.  The exact
    # kernels spend one fp32 MFMA multiply-accumulate per algorithmic one (peak 157.3); the split-operand kernels spend
    # three fp16 ones (x_hi*w_hi + x_hi*w_lo + x_lo*w_hi), so their ceiling is a third of the dense fp16 MFMA peak.
    split = is_split_kernel(dom_name)
    peak = MFMA_F16_PEAK_TFLOPS / 3.0 if split else MFMA_F32_PEAK_TFLOPS

    result = {
        "metric": baseline_metric(),
        "value": world * K / elapsed,
        "unit": "frames/s",
        "n_gpus": world, "steps": K, "warmup": Wm,
        "ms_per_step": elapsed / K * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32" if args.exact else "f32 (fp32 tensors and accumulation; each product as three fp16 MFMAs on split operands, error vs fp64 = the fp32 kernels')",
        "data": "synthetic (V256-ejecta stand-in volume, seeded random-init EnhanceNet weights)",
        "config": {"workload": "%s volume, %dx%d -> %dx%d 4x SR inference, orbit camera, temporal=%s" % (
            args.volume, low_w, low_h, 4 * low_w, 4 * low_h, "off" if args.no_temporal else "on"),
            "frames_per_rank": K, "sharding": "contiguous frame chunks per rank, no collective",
            "sequence": ("the K timed frames continue a running sequence (the last %d warm-up frames are shown again after the reset, untimed): "
                         "each timed frame = SR(t) with the ray-march of t + 1 beside it; the start of a sequence is `sequence_start`" % lead
                         if lead else "no warm-up: the timed region starts the sequence (in-line ray-march + first-frame range check inside it)"),
            "spin_kernel_forms": ops.spin_kernel_forms(),       # all-resident forms (dataflow trunk, one-launch flow fill): off when ranks share a device
            "overlap": ("render(t+1) on a side HIP stream || SR(t), released when the trunk has ended" +
                        (", kernel variant %d capped at %d ray-march waves" % (pipe.side_variant, pipe.side_waves) if pipe.side_variant == 2 else
                         ", ray-march kernel variant %d (124 registers)" % pipe.side_variant if pipe.side_variant == 5 else
                         "")) if overlap else "off",
            "conv_kernels": "exact fp32 fmaf chain (v_mfma_f32_32x32x2_f32)" if args.exact else
                            "split-operand: 3 x v_mfma_f32_32x32x16_f16 per product, fp32 accumulation (bench.py --exact = fp32 MFMA kernels); "
                            "1080p tail fused (postblock.6 + postblock.8 + finish), packed-split hand-over postblock.4 -> tail and inside the blocks"},
        **rank_keys,
        "frame_graph": ({"replays_in_timed_region": graph_replays, "untimed_prewarm_frames_beyond_warmup": graph_prewarm,
                         "per_kernel_durations": "eager pass of the same frames after the timed region"}
                        if pipe.graph else None),
        "debug_switches": switches,
        # lib/libisr_sr.so is the PRODUCT build (no isrDebug* symbol: `debug_switches` is 0 by construction); a line measured on the diagnostics build says so
        "kernel_library": {"file": os.path.basename(ops._native.SR_LIB), "diagnostics_build": ops.is_diagnostics_library()},
        "roofline": {"kernel": dom_name, "bound": "mfma", "achieved": achieved, "peak": peak,
                     "unit": "TFLOP/s", "frac": achieved / peak, "traffic": traffic,
                     "peak_source": ("dense fp16 MFMA %.0f TFLOP/s / 3 matrix products per algorithmic multiply-accumulate" % MFMA_F16_PEAK_TFLOPS)
                                    if split else "fp32 MFMA",
                     "matrix_tflops_executed": achieved * (3.0 if split else 1.0),
                     "sustained_clock_note": ("measured, not used for `peak`: a bare v_mfma_f32_32x32x16_f16 loop on changing random operands holds 1.45-1.65 GHz "
                                              "of the 2.4 GHz `peak` is priced at (zeros: 2.13 GHz; profiles/r04_mfma_valu_overlap.txt, DESIGN 4.2g; in the frame GRBM_GUI_ACTIVE gives 2.06-2.11 GHz for the three convolution kernels, profiles/r05_clock.txt)") if split else None,
                     "traffic_source": ("profiles/%s (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE, bytes per launch)" % traffic_file) if traffic else None,
                     "avg_launch_ms": dom_time / dom_launches * 1e3, "launches_per_frame": dom_launches / K,
                     "flops_per_launch": dom_flops / dom_launches},
        # every profiled kernel with ITS OWN roofline fraction (the 1080p kernels and the 480 x 270 trunk are bound differently)
        "kernels": {n: {"tflops": v[0] / v[1] / 1e12, "ms_per_frame": v[1] / K * 1e3, "launches_per_frame": v[2] / K,
                        "frac": (v[0] / v[1] / 1e12 / ((MFMA_F16_PEAK_TFLOPS / 3.0) if is_split_kernel(n)
                                                       else MFMA_F32_PEAK_TFLOPS)) if v[0] > 0 else None}      # None: no matrix work (assembly, packing, finishing)
                    for n, v in per.items()},
        # the frame's time that is NOT inside a main-stream kernel, and the host's share (an outlier run explains itself from this);
        # it needs every kernel's duration: the small kernels' pass runs with --full only (BENCH_PROFILE_SMALL=1 times them in the region)
        "frame_time": gap_accounting(elapsed / K * 1e3, per, K, host_ms)
                      if (prof_timed or pipe.graph) and (args.full or prof_small_timed) else None,
        "raymarch": {"kernel": "iso_render_gather (on a side stream under the network)" if overlap else "iso_render_gather",
                     "ms_per_frame": rm_time * 1e3, "alone_ms_per_frame": rm_alone * 1e3 if rm_alone is not None else None},
        # what the line leaves out without --full (the legs below, and the per-kernel passes behind `kernels` / `frame_time`)
        "full": bool(args.full),
    }

    if args.full and rank == 0 and world == 1:
        result["sequence_start"] = sequence_start_leg(pipe, origins, Wm, overlap, sync)
    if args.full and rank == 0 and world == 1 and args.sustained_frames > 0:
        result["sustained"] = sustained_leg(pipe, args.sustained_frames, max(64, world * K), overlap, sync)
    if args.full and rank == 0 and world == 1 and not args.exact and not args.no_exact_leg:
        result["exact_f32"] = exact_leg(pipe, origins, Wm, K, overlap, sync)
    if args.full and rank == 0 and world == 1 and not args.no_fast_mode:
        result["f16_fast_mode"] = fast_mode_leg(pipe, origins, Wm, K, overlap, sync)
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        result.update(cpu_reference_leg(args, vol, iso, net, pipe, origins[Wm], low_w, low_h, result, rm_alone))
    if rank == 0 and world == 1 and args.raymarch_large:
        result["raymarch_large"] = raymarch_large_leg(args.raymarch_large, renderer)
    return result


TRAIN_FLOPS_PER_SAMPLE_FRAME = 13.4e9      # conv forward + data gradient + weight gradient of one 32^2 -> 128^2 crop
TRAIN_OPT = dict(upsample='bilinear', reconType='residual', useBN=False, numResidualLayers=10,
                 losses="l1:mask:1,l1:ao:1,l1:normal:10,l1:depth:10,temp-l2:color:0.1",
                 lossAO=0.0, lossAmbient=0.1, lossDiffuse=0.9, lossSpecular=0.0)


def _clip_batch(torch, B, T, crop, seed, device):
    g = torch.Generator().manual_seed(seed)
    inp = torch.rand(B, T, 5, crop, crop, generator=g); inp[:, :, 0] = inp[:, :, 0] * 2 - 1
    flow = (torch.rand(B, T, 2, crop, crop, generator=g) - 0.5) * 0.05
    tgt = torch.rand(B, T, 6, 4 * crop, 4 * crop, generator=g); tgt[:, :, 0] = tgt[:, :, 0] * 2 - 1
    return tuple(t.to(device) for t in (inp, flow, tgt))


def run_train(args, job):
    """BASELINE config #3: the training step of mainVideoUnshaded.py:397-473 data-parallel over
    the ranks.  Global batch fixed (strong scaling), rank-0 broadcast of the weights, one flat all-reduce of the
    911 046 fp32 gradients per step -- on the GPU captured with the whole step in ONE HIP graph."""
    import torch
    import torch.distributed as dist
    from isosurfacesuperresolution_amd import losses, models, train
    world, rank, dev = job.world, job.rank, job.device
    B, T, crop = args.train_batch, args.train_frames, args.train_crop
    assert B % world == 0, "--train-batch must be divisible by the number of ranks"
    clips_per_rank = B // world
    opt = argparse.Namespace(**TRAIN_OPT)
    torch.manual_seed(124)                                              # mainVideoUnshaded.py:157
    with contextlib.redirect_stdout(sys.stderr):
        net = models.createNetwork('EnhanceNet', 4, 101, [0, 1, 2, 3, 4], 6, opt).to(dev)
        crit = losses.LossNetUnshaded(dev, 5, 6, 4 * crop, crop // 2, opt).to(dev)
    # FlatAdam: torch.optim.Adam's update over one flat buffer in one launch; its gradient buffer is the all-reduce bucket
    optim, _ = train.make_optimizer(net, capturable=(dev == "cuda"), flat=True)
    trainer = train.DataParallelTrainer(net, crit, optim)
    batch = _clip_batch(torch, clips_per_rank, T, crop, 1000 + rank, dev)
    from isosurfacesuperresolution_amd import ops
    # which kernel family every convolution of ONE step goes to (algorithmic flops; shapes decide, so one eager step tells)
    ops.FLOP_TALLY = {}
    trainer.step(batch, initial_image="zero")
    tally, ops.FLOP_TALLY = ops.FLOP_TALLY, None
    graphed = dev == "cuda" and (world == 1 or job.backend == "nccl")     # gloo collectives cannot be captured
    step, step_kind = make_train_step(trainer, batch, graphed, sync=torch.cuda.synchronize if dev == "cuda" else (lambda: None))
    K, Wm = args.steps, args.warmup
    loss = None
    for _ in range(Wm):
        loss = step()
    job.sync()
    t0 = time.perf_counter()
    for _ in range(K):
        loss = step()
    job.sync()
    elapsed = job.max_over_ranks(time.perf_counter() - t0)
    loss = float(loss)
    if args.dump_outputs and rank == 0 and K > 0:
        # the last timed step's loss and the weights it left (before the eager per-kernel step below moves them again)
        sys.stderr.write("bench.py: --dump-outputs %s\n" % json.dumps(dump_outputs(args.dump_outputs, {
            "loss": torch.tensor([loss], dtype=torch.float64), "parameters": torch.cat([p.detach().reshape(-1) for p in net.parameters()])})))
    # the collective on its own: the flat gradient bucket, as in the step
    allreduce = None
    if world > 1:
        n = 20
        for _ in range(3):
            dist.all_reduce(trainer.bucket)
        job.sync()
        t1 = time.perf_counter()
        for _ in range(n):
            dist.all_reduce(trainer.bucket)
        job.sync()
        allreduce = {"bytes": trainer.numel * 4, "us": job.max_over_ranks(time.perf_counter() - t1) / n * 1e6,
                     "buckets": 1, "backend": "RCCL" if job.backend == "nccl" else job.backend}
    flops = TRAIN_FLOPS_PER_SAMPLE_FRAME * (crop / 32.0) ** 2 * B * T
    achieved = flops / (elapsed / K) / 1e12
    # per-kernel fractions of the convolution launchers that carry dispatch-packet events -- forward and data-gradient convolutions and, since
    # round 6, the split-operand weight gradient (conv3x3_wgrad_split_kernel: one entry per 64 x 64 channel block and layer): ONE eager step
    # after the timed region (a replayed graph has no per-dispatch events)
    train_kernels = None
    if dev == "cuda":
        torch.cuda.synchronize()
        ops.profile_enable(True)
        trainer.step(batch, initial_image="zero")
        torch.cuda.synchronize()
        kernel_tally = tally_kernels(ops.profile_records())
        ops.profile_enable(False)
        train_kernels = {n: {"tflops": v[0] / v[1] / 1e12, "ms_per_step": v[1] * 1e3, "launches_per_step": v[2],
                             "frac": v[0] / v[1] / 1e12 / ((MFMA_F16_PEAK_TFLOPS / 3.0) if is_split_kernel(n) else MFMA_F32_PEAK_TFLOPS)}
                         for n, v in kernel_tally.items() if v[1] > 0 and v[0] > 0}
    # Roofline per kernel family, weighted by the flops each family carries: the time the step's convolutions would take
    # at each family's own ceiling is sum(flops_f / peak_f); the step's ceiling is total / that time (a harmonic mean).
    peaks = {"split": MFMA_F16_PEAK_TFLOPS / 3.0, "exact": MFMA_F32_PEAK_TFLOPS, "bf16": MFMA_F16_PEAK_TFLOPS}
    tally_total = sum(tally.values()) or 1.0
    shares = {k: v / tally_total for k, v in tally.items()}
    peak = 1.0 / sum(share / peaks[k] for k, share in shares.items()) if shares else MFMA_F32_PEAK_TFLOPS
    dtype = "f32" if not shares.get("split") else (
        "f32 (fp32 tensors and accumulation; %.0f %% of the step's conv flops as three fp16 MFMAs per product on split operands, error vs "
        "fp64 = the fp32 kernels'; the rest on fp32 MFMA)" % (100 * shares["split"]))
    result = {
        "metric": "training clips/sec (mainVideoUnshaded.py step, BASELINE config #3), data-parallel over the GPUs of one node",
        "value": B * K / elapsed, "unit": "clips/s", "n_gpus": world, "steps": K, "warmup": Wm,
        "ms_per_step": elapsed / K * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": dtype, "data": "synthetic (random clips of the dataset's shapes, seeded random-init EnhanceNet)",
        "config": {"workload": "EnhanceNet training step: global batch %d clips x %d frames, %dx%d -> %dx%d crops, "
                               "losses l1:mask:1,l1:ao:1,l1:normal:10,l1:depth:10,temp-l2:color:0.1, Adam 1e-4" % (B, T, crop, crop, 4 * crop, 4 * crop),
                   "clips_per_rank": clips_per_rank, "spin_kernel_forms": ops.spin_kernel_forms() if dev == "cuda" else None, "parallelism": "dp%d, one flat %.2f MB gradient all-reduce per step" % (world, trainer.numel * 4 / 1e6),
                   "step": step_kind},
        **job.rank_keys(), "allreduce": allreduce, "loss": loss,
        "roofline": {"kernel": "all convolutions of the step (forward + data gradient + weight gradient), whole-step time", "bound": "mfma",
                     "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
                     "traffic": None, "flops_per_step": flops,
                     "flop_share_by_kernel_family": shares,
                     "peak_source": "flop-weighted over the kernel families of one step (ops.FLOP_TALLY): split-operand kernels against dense fp16 "
                                    "MFMA %.0f / 3 products, exact kernels against fp32 MFMA %.1f TFLOP/s; peak = 1 / sum(share / family peak)"
                                    % (MFMA_F16_PEAK_TFLOPS, MFMA_F32_PEAK_TFLOPS),
                     "matrix_tflops_executed": achieved * sum(shares.get(k, 0.0) * (3.0 if k == "split" else 1.0) for k in shares),
                     "kernels": train_kernels,
                     "note": "`achieved` divides the step's algorithmic conv flops by the WHOLE step (loss, warp, Adam, all-reduce "
                             "included), so it understates the kernels; `kernels` = the forward / data-gradient convolution launches of one "
                             "eager step after the timed region with their own fractions; profiles/r04_train_kernel_stats.csv has every kernel"},
        "cpu_baseline": None,
    }
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        cores = host_cores()
        torch.set_num_threads(cores)
        torch.manual_seed(124)
        with contextlib.redirect_stdout(sys.stderr):
            cnet = models.createNetwork('EnhanceNet', 4, 101, [0, 1, 2, 3, 4], 6, opt)
            ccrit = losses.LossNetUnshaded("cpu", 5, 6, 4 * crop, crop // 2, opt)
        coptim, _ = train.make_optimizer(cnet)
        cb = _clip_batch(torch, 2, T, crop, 1000, "cpu")
        train.train_step(cnet, ccrit, coptim, cb, initial_image="zero")
        t1 = time.perf_counter()
        n = 3
        for _ in range(n):
            train.train_step(cnet, ccrit, coptim, cb, initial_image="zero")
        dt = (time.perf_counter() - t1) / n
        result["cpu_baseline"] = {"value": 2 / dt, "unit": "clips/s", "cores": cores, "kind": "port",
                                  "sample": "%d steps of 2 clips x %d frames on CPU PyTorch (%d threads), %.2f s per step" % (n, T, cores, dt)}
    return result


def make_train_step(trainer, batch, want_graph, sync=lambda: None):
    """-> (step callable, description).  ``want_graph``: capture the whole step (with its all-reduce) in ONE HIP graph.  A
    failed capture (e.g. an RCCL build that cannot capture its all-reduce) must not end the run, and nothing may re-execute
    a process that has touched the GPU: fall back to the eager step IN THIS PROCESS and say so in the line."""
    eager = lambda: trainer.step(batch, initial_image="zero")
    if not want_graph:
        return eager, "eager"
    try:
        step_fn = trainer.graphed(batch, initial_image="zero")
        return (lambda: step_fn(batch)), "one HIP graph (forward x T, backward through time, deferred weight gradients, all-reduce, Adam)"
    except Exception as exc:      # noqa: BLE001 -- whatever the capture raised
        sync()
        trainer.zero_grad()
        msg = str(exc).splitlines()[0][:160] if str(exc) else ""
        return eager, "eager (capture failed: %s: %s)" % (type(exc).__name__, msg)


TILE_SPLITS = {1: (1, 1, 1), 2: (2, 1, 1), 4: (2, 2, 1), 8: (2, 2, 2)}


def run_tiled(args, job, make_local_renderer=None):
    """BASELINE config #5: a volume too large to want on one GPU, split in object space, one tile per
    rank.  Every rank generates ONLY its tile of the global lattice (one scalar max / bbox reduction between ranks),
    ray-marches the full low-resolution image against it, one all-gather + nearest-hit composite gives every rank the
    frame (bit-identical to the unsplit render), the 4x network runs in screen strips with a second all-gather.
    ``make_local_renderer(tile) -> object with .render(tensor[H,W,12], origin)``: CPU rehearsals of the exchange (tests)."""
    import numpy as np
    import torch
    import torch.distributed as dist
    from isosurfacesuperresolution_amd import models, parallel_render as PR, parallel_sr, volumes as V
    from isosurfacesuperresolution_amd.inference import LoadedModel
    from isosurfacesuperresolution_amd.pipeline import default_shading
    world, rank, dev = job.world, job.rank, job.device
    assert world in TILE_SPLITS, "--mode tiled runs on 1, 2, 4 or 8 ranks"
    n = args.tiled_n
    low_w, low_h = (int(v) for v in (args.low or "960x540").split("x"))

    def reducer(op):
        def fn(a):
            if world == 1:
                return a
            t = torch.from_numpy(np.ascontiguousarray(a)).to(job.coll_device)
            dist.all_reduce(t, op=op)
            return t.cpu().numpy()
        return fn
    t0 = time.perf_counter()
    tiles = PR.generate_tiles(V.EjectaField(n, seed=1024 if n == 1024 else 272), TILE_SPLITS[world], ranks=[rank],
                              reduce_max=reducer(dist.ReduceOp.MAX), reduce_min=reducer(dist.ReduceOp.MIN))
    tile = tiles[rank]
    t_gen = time.perf_counter() - t0
    if make_local_renderer is not None:
        local = make_local_renderer(tile)
        renderer = None
    else:
        from isosurfacesuperresolution_amd.inference import DirectRenderer
        renderer = DirectRenderer()
        for c, v in (("cameraLookAt", "0,0,0"), ("cameraUp", "0,1,0"), ("cameraFoV", "30.000"), ("isovalue", "0.340"), ("aosamples", "0"),
                     ("resolution", "%d,%d" % (low_w, low_h)), ("viewport", "0,0,%d,%d" % (low_w, low_h)),
                     ("cameraOrigin", V.fmt3(V.orbit_camera(-1)))):
            renderer.send_command(c, v)
        t0 = time.perf_counter()
        renderer.load_tile(tile)
        t_load = time.perf_counter() - t0

        class _Local:
            def render(self, tensor, origin, stream=None):
                renderer.send_command("cameraOrigin", V.fmt3(origin))
                renderer.render_async(tensor, stream if stream is not None else torch.cuda.current_stream())
        local = _Local()
    del tiles
    opt = argparse.Namespace(upsample='bilinear', reconType='residual', useBN=False, numResidualLayers=10)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(sys.stderr):
        net = models.createNetwork('EnhanceNet', 4, 101, [0, 1, 2, 3, 4], 6, opt)
    lm = LoadedModel.from_model(net, dev, parameters={"initialImage": "zero"})
    # screen tiles of the super-resolution: the (rows x columns) grid whose largest tile + halo is smallest (8 ranks at 960 x 540: 2 x 4,
    # 1.31 x a rank's share against 1.71 x with strips); BENCH_TILED_GRID=strips forces horizontal strips
    sr_grid = None if os.environ.get("BENCH_TILED_GRID", "auto") == "strips" else parallel_sr.best_grid(world, low_h, low_w)
    sr = parallel_sr.StripSuperResolution(lm, default_shading(dev, 30.0), grid=sr_grid)
    sr_grid = sr_grid or (world, 1)
    K, Wm = args.steps, args.warmup
    # render(t+1) + all-gather + composite on a side stream beside SR(t), released when SR(t)'s trunk is enqueued (as the default
    # mode's pipeline does); --no-overlap: one after the other
    overlap = dev == "cuda" and not args.no_overlap
    release = os.environ.get("BENCH_TILED_RELEASE", "trunk")               # trunk | start: where in SR(t) the next frame is released

    def render_fn(tensor, key, stream):
        if renderer is not None:
            local.render(tensor, V.orbit_camera(key), stream)
        else:
            local.render(tensor, V.orbit_camera(key))
    source = PR.PrefetchedComposite(render_fn, low_h, low_w, dev)
    sr_events = []

    def stamp():
        return torch.cuda.current_stream().record_event(torch.cuda.Event(enable_timing=True)) if dev == "cuda" else time.perf_counter()

    def frame(k, timed, last):
        """``last``: nothing is prefetched behind this frame (exactly K renders inside the timed region)."""
        comp = source.take(k)
        ahead = overlap and not last
        if ahead and release == "start":
            source.start(k + 1)
        a = stamp()
        rgb, raw = sr.frame(comp, after_trunk=(lambda: source.start(k + 1)) if (ahead and release != "start") else None)
        if timed:
            sr_events.append((a, stamp()))
        return comp, rgb

    for k in range(Wm):
        frame(k - Wm, False, k + 1 == Wm)
    if world > 1:
        # a silently no-op all-gather must not pass: every rank's own hit count travels through a DIFFERENT collective
        # (an all-reduce of a one-hot vector) and must equal the hit count of the slice the all-gather delivered for it
        if dev == "cuda":
            torch.cuda.synchronize()
        check_mine = torch.empty_like(source.local)
        render_fn(check_mine, -1, None)
        check_all = torch.empty_like(source.gathered)
        dist.all_gather_into_tensor(check_all.view(world * low_h, low_w, 12), check_mine)
        own = torch.zeros(world, dtype=torch.float64, device=job.coll_device)
        own[rank] = float((check_mine[..., 3] == 1).sum().item())
        dist.all_reduce(own)
        got = [float((check_all[r][..., 3] == 1).sum().item()) for r in range(world)]
        assert got == own.tolist(), "all-gather of the G-buffers delivered %s hit pixels per rank, the ranks rendered %s" % (got, own.tolist())
        del check_mine, check_all
    source.record(True)
    sr.reset()
    from isosurfacesuperresolution_amd import ops
    if dev == "cuda":
        ops.profile_enable(True)
    job.sync()
    t0 = time.perf_counter()
    for k in range(K):
        comp, rgb = frame(k, True, k + 1 == K)
    job.sync()
    elapsed = job.max_over_ranks(time.perf_counter() - t0)
    if dev == "cuda":
        torch.cuda.synchronize()
    if args.dump_outputs and rank == 0 and K > 0:
        sys.stderr.write("bench.py: --dump-outputs %s\n" % json.dumps(dump_outputs(args.dump_outputs, {"rgb": rgb, "gbuffer": comp})))
    # per-phase times from events on the stream each phase ran on (no host synchronisation inside the timed region)
    phases = dict(zip(("render", "allgather", "composite"), (v * 1e-3 for v in source.phase_ms())))
    phases["sr_strip_and_allgather"] = sum(a.elapsed_time(b) * 1e-3 if dev == "cuda" else b - a for a, b in sr_events)
    ms = {name: job.max_over_ranks(v) / K * 1e3 for name, v in phases.items()}
    hits = int((comp[..., 3] == 1).sum().item())
    # roofline of the dominant kernel: the strip's convolutions (same formula as the default mode)
    y0, y1, x0, x1 = parallel_sr.tile_bounds(low_h, low_w, sr_grid, rank)
    rows, cols = min(low_h, y1 + sr.halo) - max(0, y0 - sr.halo), min(low_w, x1 + sr.halo) - max(0, x0 - sr.halo)
    strip_flops = 564.5e9 * (cols * rows) / (480.0 * 270.0)              # SURVEY.md App. B, scaled to this rank's tile (halo included)
    if dev == "cuda":
        torch.cuda.synchronize()
        per = tally_kernels(ops.profile_records())
        ops.profile_enable(False)
        dom_name, (dom_flops, dom_time, dom_launches) = max(((n, v) for n, v in per.items() if v[0] > 0), key=lambda kv: kv[1][1])
        split = is_split_kernel(dom_name)
        peak = MFMA_F16_PEAK_TFLOPS / 3.0 if split else MFMA_F32_PEAK_TFLOPS
        achieved = dom_flops / dom_time / 1e12
        roofline = {"kernel": dom_name, "bound": "mfma", "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
                    "traffic": None, "avg_launch_ms": dom_time / dom_launches * 1e3, "launches_per_frame": dom_launches / K,
                    "flops_per_launch": dom_flops / dom_launches,
                    "peak_source": ("dense fp16 MFMA %.0f TFLOP/s / 3 matrix products per algorithmic multiply-accumulate" % MFMA_F16_PEAK_TFLOPS)
                                   if split else "fp32 MFMA",
                    "kernels": {n: {"tflops": v[0] / v[1] / 1e12, "ms_per_frame": v[1] / K * 1e3, "launches_per_frame": v[2] / K}
                                for n, v in per.items()}}
    else:
        t_sr = phases["sr_strip_and_allgather"] / K
        achieved = strip_flops / max(t_sr, 1e-9) / 1e12
        roofline = {"kernel": "CPU rehearsal (BENCH_DEVICE=cpu): no HIP kernel ran; the strip's convolutions through PyTorch CPU ops",
                    "bound": "mfma", "achieved": achieved, "peak": MFMA_F16_PEAK_TFLOPS / 3.0, "unit": "TFLOP/s",
                    "frac": achieved / (MFMA_F16_PEAK_TFLOPS / 3.0), "traffic": None, "flops_per_strip": strip_flops}
    cpu_baseline = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu_baseline = tiled_cpu_leg(tile, low_w, low_h, net, dev)
    return {
        "metric": "frames/sec (object-space tiled %d^3 render + all-gather composite + 4x SR in screen strips, BASELINE config #5)" % n,
        "value": K / elapsed, "unit": "frames/s", "n_gpus": world, "steps": K, "warmup": Wm,
        "ms_per_step": elapsed / K * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic (ejecta %d^3 stand-in volume generated tile-wise, seeded random-init EnhanceNet weights)" % n,
        "config": {"workload": "%d^3 volume in %s object-space tiles, %dx%d -> %dx%d, temporal on" % (
                       n, "x".join(str(v) for v in TILE_SPLITS[world]), low_w, low_h, 4 * low_w, 4 * low_h),
                   "sharding": "one tile per rank; all-gather of %.1f MB G-buffers + nearest-hit composite; SR in %d x %d screen tiles with a 24-px halo "
                               "(largest tile + halo = %.2f x a rank's share) + all-gather"
                               % (low_w * low_h * 48 / 1e6, sr_grid[0], sr_grid[1], parallel_sr.extended_area(low_h, low_w, sr_grid) * world / float(low_h * low_w)),
                   "overlap": ("render + all-gather + composite of frame t+1 on a side HIP stream || SR(t), released at SR(t)'s %s" % release)
                              if overlap else "none",
                   "spin_kernel_forms": ops.spin_kernel_forms() if dev == "cuda" else None},
        **job.rank_keys(),
        "phases_ms_max_over_ranks": ms,
        "tile": {"generate_s": t_gen, "voxels": [int(v) for v in tile["data"].shape[::-1]]},
        "hit_pixels": hits, "rgb_mean": float(rgb.mean().item()),
        "roofline": roofline, "cpu_baseline": cpu_baseline,
    }


def tiled_cpu_leg(tile, low_w, low_h, net, dev):
    """CPU baseline of the tiled mode on a bounded sample: ONE frame -- the oracle ray-marches the (single) tile at the low
    resolution on the host cores, the same network super-resolves the whole frame on CPU PyTorch."""
    import torch
    from isosurfacesuperresolution_amd import models, volumes as V, utils
    from isosurfacesuperresolution_amd.inference import LoadedModel
    from isosurfacesuperresolution_amd.pipeline import default_shading
    from oracle import iso_oracle
    cores = host_cores()
    torch.set_num_threads(cores)
    t0 = time.perf_counter()
    ov = iso_oracle.OracleVolume(tile["data"], tile=tile)
    t_load = time.perf_counter() - t0
    q, last = V.quantize3(V.orbit_camera(0)), V.quantize3(V.orbit_camera(-1))
    p = iso_oracle.make_params(low_w, low_h, origin=q, fov=30.0, isovalue=0.34, last_origin=last)
    t0 = time.perf_counter()
    ref, _ = iso_oracle.render(ov, p, threads=cores, with_stats=False)
    t_render = time.perf_counter() - t0
    opt = argparse.Namespace(upsample='bilinear', reconType='residual', useBN=False, numResidualLayers=10)
    with contextlib.redirect_stdout(sys.stderr):
        cpu_net = models.createNetwork('EnhanceNet', 4, 101, [0, 1, 2, 3, 4], 6, opt)
    cpu_net.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
    cpu_model = LoadedModel.from_model(cpu_net.eval(), "cpu", parameters={"initialImage": "zero"})
    low = torch.from_numpy(ref).permute(2, 0, 1).unsqueeze(0)
    t0 = time.perf_counter()
    raw = cpu_model.inference(low, None)
    raw = torch.cat([raw[:, 0:1].clamp(-1, 1), utils.ScreenSpaceShading.normalize(raw[:, 1:4], dim=1), raw[:, 4:].clamp(0, 1)], dim=1)
    default_shading("cpu", 30.0)(raw)
    t_sr = time.perf_counter() - t0
    return {"value": 1.0 / (t_render + t_sr), "unit": "frames/s", "cores": cores, "kind": "port",
            "sample": "1 frame: oracle ray-march of the tile %dx%d (%.3f s, OpenMP %d threads; brick build %.1f s not counted) + PyTorch CPU "
                      "EnhanceNet and shading of the whole %dx%d frame (%.3f s, %d threads)" % (low_w, low_h, t_render, cores, t_load,
                                                                                              4 * low_w, 4 * low_h, t_sr, cores)}


SUSTAINED_WINDOW = 100


def sustained_summary(n_frames, elapsed_s, window_ms, window=SUSTAINED_WINDOW, guards="clean"):
    """The `sustained` object of the bench line from its raw measurements (tests/test_bench_modes_cpu.py checks this shape): the whole run's
    rate by the host clock between two synchronisations, and the spread of the per-window rates (device events every ``window`` frames)."""
    rates = sorted(window * 1e3 / ms for ms in window_ms if ms > 0)
    med = (rates[len(rates) // 2] if len(rates) % 2 else 0.5 * (rates[len(rates) // 2 - 1] + rates[len(rates) // 2])) if rates else None
    return {"frames": n_frames, "seconds": elapsed_s, "value": n_frames / elapsed_s, "unit": "frames/s", "ms_per_step": elapsed_s / n_frames * 1e3,
            "window_frames": window, "windows": len(rates),
            "window_frames_per_s": {"min": rates[0] if rates else None, "median": med, "max": rates[-1] if rates else None},
            "guards": guards,
            "note": "the same pipeline as `value` (render(t+1) beside SR(t), temporal recurrence) run for `frames` more frames after the timed "
                    "region, the orbit repeated; `value` stays what --steps asked for.  The K timed frames come out 2-4 % slower per frame than "
                    "this run: the dispatch-packet events on the convolution launches that `roofline.achieved` is measured with cost 1.4 %, "
                    "a 20-30 frame window after an idle gap 1.2 % (profiles/r06_timed_region_ab.txt)"}


def sequence_start_leg(pipe, origins, Wm, overlap, sync):
    """What the FIRST frame of a temporal sequence costs (outside the timed region, which runs in steady state): nothing rendered ahead --
    the ray-march runs in line --, no previous output, and the first frame's range check waits for the device (loadedmodel.guarded_forward).
    Median of five starts, host clock around a synchronised frame."""
    ms = []
    for _ in range(5):
        pipe.reset()
        sync()
        t0 = time.perf_counter()
        pipe.frame(origins[Wm], origins[Wm + 1] if overlap else None)
        sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    pipe.reset()
    return {"first_frame_ms": sorted(ms)[2], "first_frame_ms_all": [round(v, 3) for v in ms],
            "note": "one synchronised first frame after pipe.reset(): in-line ray-march + SR + first-frame range check (+ the next frame's ray-march "
                    "on the side stream); outside the K timed frames, which continue a running sequence"}


def sustained_leg(pipe, n_frames, orbit, overlap, sync):
    """a sturdier number beside the K timed frames -- the same pipeline for >= 2 000 frames (about 3.5 s), whole-run
    frames/s plus min / median / max over 100-frame windows (one device event per window on the main stream, read at the end: no host
    synchronisation inside the run), and the guard words (range maxima, the spin kernels' error words) looked at when it ends."""
    import torch
    from isosurfacesuperresolution_amd import ops, volumes as V
    n_frames = max(SUSTAINED_WINDOW, (n_frames // SUSTAINED_WINDOW) * SUSTAINED_WINDOW)
    cams = [V.orbit_camera(k, K=orbit) for k in range(orbit + 1)]
    pipe.reset()
    for k in range(3):
        pipe.frame(cams[k], cams[k + 1] if overlap else None)
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(n_frames // SUSTAINED_WINDOW + 1)]
    sync()
    t0 = time.perf_counter()
    marks[0].record()
    for k in range(n_frames):
        c = (3 + k) % orbit
        pipe.frame(cams[c], cams[c + 1] if overlap and k + 1 < n_frames else None)
        if (k + 1) % SUSTAINED_WINDOW == 0:
            marks[(k + 1) // SUSTAINED_WINDOW].record()
    sync()
    elapsed = time.perf_counter() - t0
    guards = "clean"
    try:
        ops.guards_flush("cuda")          # the last frame's guard words (every earlier frame's were polled by the frame after it)
        ops.trunk_check()
        if ops.any_hot("cuda"):
            guards = "a producer came within range of the fp16 split's overflow: its consumers were re-routed to the exact kernels"
    except RuntimeError as e:             # a spin kernel gave up on a neighbour: the number is not a measurement of the default path
        guards = "FAILED: %s" % e
    window_ms = [marks[i].elapsed_time(marks[i + 1]) for i in range(len(marks) - 1)]
    pipe.reset()
    return sustained_summary(n_frames, elapsed, window_ms, guards=guards)


def exact_leg(pipe, origins, Wm, K, overlap, sync):
    """The same frames with every convolution on the exact k-ordered fp32 fmaf-chain kernels (v_mfma_f32_32x32x2_f32;
    ``ops.SPLIT_F16 = False``, what ``--exact`` times as the headline), OUTSIDE the timed region of ``value``: the
    IEEE-fp32 number next to the split-operand one, plus how far the two paths' frames are apart."""
    import torch
    from isosurfacesuperresolution_amd import ops
    n = min(K, 10)

    def run(collect):
        pipe.reset()
        for k in range(min(Wm, 3)):
            pipe.frame(origins[k], origins[k + 1] if overlap else None)
        pipe.reset()
        # the timing run continues a running sequence like the headline's timed region; the collecting run compares a sequence's FIRST frame
        for k in range(Wm - (0 if collect else min(Wm, 2)), Wm):
            pipe.frame(origins[k], origins[k + 1] if overlap else None)
        sync()
        t0 = time.perf_counter()
        first = None
        for k in range(n):
            _, raw = pipe.frame(origins[Wm + k], origins[Wm + k + 1] if overlap else None)
            if collect and k == 0:
                first = raw.clone()
        sync()
        return time.perf_counter() - t0, first

    _, split_first = run(True)
    ops.SPLIT_F16 = False
    try:
        _, exact_first = run(True)
        elapsed, _ = run(False)
    finally:
        ops.SPLIT_F16 = True
    return {"value": n / elapsed, "unit": "frames/s", "ms_per_step": elapsed / n * 1e3, "frames": n,
            "dtype": "f32 (exact k-ordered fmaf chain on v_mfma_f32_32x32x2_f32)",
            "max_abs_diff_vs_split_first_frame": float((split_first - exact_first).abs().max().item()),
            "note": "separate from `value`: the same frames with ops.SPLIT_F16 = False (bench.py --exact makes it the headline)"}


def fast_mode_leg(pipe, origins, Wm, K, overlap, sync):
    """The same frames with the convolutions in the fp16 fast mode (csrc/sr_conv_f16.hip), OUTSIDE the timed region of
    the headline number and reported separately: it is not the parity path, its quality figure is a PSNR against the
    fp32 frames."""
    import torch
    from isosurfacesuperresolution_amd import ops
    n = min(K, 20)

    def run(collect):
        pipe.reset()
        frames = []
        for k in range(Wm):
            pipe.frame(origins[k], origins[k + 1] if overlap else None)
        pipe.reset()
        # (timing run: a running sequence, like the headline's timed region; collecting run: the sequence from its first frame)
        for k in range(Wm - (0 if collect else min(Wm, 2)), Wm):
            pipe.frame(origins[k], origins[k + 1] if overlap else None)
        sync()
        t0 = time.perf_counter()
        for k in range(n):
            rgb, _ = pipe.frame(origins[Wm + k], origins[Wm + k + 1] if overlap else None)
            if collect:
                frames.append(rgb.clone())
        sync()
        return time.perf_counter() - t0, frames

    _, ref = run(True)                       # fp32 frames of the same camera path
    ops.FAST_F16 = True
    try:
        _, fast = run(True)
        elapsed, _ = run(False)
    finally:
        ops.FAST_F16 = False
    mse = [((a - b) ** 2).mean().item() for a, b in zip(fast, ref)]
    psnr = [10.0 * math.log10(1.0 / m) if m > 0 else 100.0 for m in mse]
    return {"value": n / elapsed, "unit": "frames/s", "ms_per_step": elapsed / n * 1e3, "frames": n,
            "dtype": "f16 operands, f32 accumulation and tensors (convolutions with more than 8 output channels)",
            "psnr_rgb_vs_f32_db_first": psnr[0], "psnr_rgb_vs_f32_db_min": min(psnr), "psnr_rgb_vs_f32_db_last": psnr[-1],
            "note": "separate from `value`: not the 1e-4 parity path (and no longer faster than it: the default's dataflow trunk, packed activations and fused tail have no fp16-operand counterpart -- this leg launches the network layer by layer); the recurrence feeds its own output back, so the PSNR is that of the whole temporal sequence (random-init weights: rounding differences grow from frame to frame)"}


def raymarch_large_leg(spec, renderer):
    """The ray-march kernel on its own on a volume larger than L2 + Infinity Cache ("for 512^3 the
    HBM figure becomes meaningful"): time from the dispatch-packet events, algorithmic bytes = bricks the CPU
    restatement touches x 2048 B + W*H*48 B (counted here the way the cpu_baseline leg does), one frame."""
    import torch
    from isosurfacesuperresolution_amd import volumes as V
    from oracle import iso_oracle
    name, res = spec.split("@")
    w, h = (int(v) for v in res.split("x"))
    n = int(name.replace("cloud", "").replace("ejecta", ""))
    vol = V.cloud(n) if name.startswith("cloud") else V.ejecta(n)
    iso = 0.30 if name.startswith("cloud") else 0.34
    renderer.load_dense(vol)
    for c, v in [("cameraLookAt", "0,0,0"), ("cameraUp", "0,1,0"), ("cameraFoV", "30.000"), ("isovalue", "%5.3f" % iso),
                 ("aosamples", "0"), ("resolution", "%d,%d" % (w, h)), ("viewport", "0,0,%d,%d" % (w, h))]:
        renderer.send_command(c, v)
    renderer.set_kernel_variant(0)
    out = torch.empty((h, w, 12), dtype=torch.float32, device="cuda")
    origins = [V.quantize3(V.orbit_camera(k)) for k in range(12)]
    for k in range(2):
        renderer.send_command("cameraOrigin", V.fmt3(origins[k]))
        renderer.render_direct(out)
    renderer.profile_enable(True)
    for k in range(2, 12):
        renderer.send_command("cameraOrigin", V.fmt3(origins[k]))
        renderer.render_async(out, torch.cuda.current_stream())
    torch.cuda.synchronize()
    ms = renderer.profile_times_ms()
    renderer.profile_enable(False)
    t = sum(ms) / len(ms) * 1e-3
    cores = host_cores()
    ov = iso_oracle.OracleVolume(vol)
    p = iso_oracle.make_params(w, h, origin=origins[11], fov=30.0, isovalue=float("%5.3f" % iso), last_origin=origins[10])
    ref, stats = iso_oracle.render(ov, p, threads=cores)
    gbuf = out.cpu().numpy()
    bytes_alg = stats["bricks_touched"] * 2048 + w * h * 48
    return {"volume": name, "resolution": "%dx%d" % (w, h), "kernel": "iso_render_gather", "ms_per_frame": t * 1e3,
            "bricks_touched": stats["bricks_touched"], "samples": stats["samples"], "algorithmic_bytes": bytes_alg,
            "achieved_GBps": bytes_alg / t / 1e9, "frac_of_8TBps": bytes_alg / t / 8e12, "samples_per_s": stats["samples"] / t,
            "mask_mismatches_vs_cpu": int((gbuf[..., 3] != ref[..., 3]).sum())}


def host_cores():
    """CPU cores this process may actually use (cgroup quota, then affinity, then cpu_count)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()
        if quota != "max":
            n = min(n, max(1, int(float(quota) / float(period) + 0.5)))
    except (OSError, ValueError):
        pass
    return min(n, int(os.environ.get("BENCH_CPU_THREADS", "16")))


def baseline_metric():
    """The metric string of BASELINE.json (kept verbatim so that the line can be matched against it)."""
    try:
        with open(os.path.join(ROOT, "BASELINE.json")) as f:
            return json.load(f)["metric"]
    except (OSError, KeyError, ValueError):
        return "frames/sec (render+4xSR) at 256^3->1080p, 1/2/4/8 GPU; PSNR vs ref"


def cpu_reference_leg(args, vol, iso, net, pipe, origin, low_w, low_h, result, rm_time):
    """CPU baseline (the oracle = a port of the reference's CPU path, timed on this box's host
    cores on a bounded sample: one frame) and PSNR of the GPU frame against it."""
    import numpy as np
    import torch
    from isosurfacesuperresolution_amd import models, volumes as V, utils
    from isosurfacesuperresolution_amd.inference import LoadedModel
    from isosurfacesuperresolution_amd.pipeline import default_shading
    from oracle import iso_oracle

    cores = host_cores()
    torch.set_num_threads(cores)
    ov = iso_oracle.OracleVolume(vol)
    q = V.quantize3(origin)
    p = iso_oracle.make_params(low_w, low_h, origin=q, fov=30.0, isovalue=float("%5.3f" % iso))
    t0 = time.perf_counter()
    ref, stats = iso_oracle.render(ov, p, threads=cores)
    t_render = time.perf_counter() - t0
    opt = argparse.Namespace(upsample='bilinear', reconType='residual', useBN=False, numResidualLayers=10)
    with contextlib.redirect_stdout(sys.stderr):
        cpu_net = models.createNetwork('EnhanceNet', 4, 101, [0, 1, 2, 3, 4], 6, opt)
    cpu_net.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
    cpu_model = LoadedModel.from_model(cpu_net.eval(), "cpu", parameters={"initialImage": "zero"})
    low = torch.from_numpy(ref).permute(2, 0, 1).unsqueeze(0)
    t0 = time.perf_counter()
    raw = cpu_model.inference(low, None)
    raw = torch.cat([raw[:, 0:1].clamp(-1, 1), utils.ScreenSpaceShading.normalize(raw[:, 1:4], dim=1),
                     raw[:, 4:].clamp(0, 1)], dim=1)
    rgb_cpu = default_shading("cpu", 30.0)(raw)
    t_sr = time.perf_counter() - t0
    # a few more frames of the same temporal sequence (flow fill + warp included), so that the sample is ~10 s
    shade_cpu = default_shading("cpu", 30.0)
    n_frames, prev, last = 1, raw, q
    cpu_frames = [(origin, ref, raw)]                       # (camera, oracle G-buffer, CPU network output) per frame of the sample
    for k in range(1, max(1, args.cpu_frames)):
        qk = V.quantize3(V.orbit_camera(k))
        pk = iso_oracle.make_params(low_w, low_h, origin=qk, fov=30.0, isovalue=float("%5.3f" % iso), last_origin=last)
        t0 = time.perf_counter()
        gk, _ = iso_oracle.render(ov, pk, threads=cores, with_stats=False)
        t_render += time.perf_counter() - t0
        t0 = time.perf_counter()
        rk = cpu_model.inference(torch.from_numpy(gk).permute(2, 0, 1).unsqueeze(0), prev)
        prev = torch.cat([rk[:, 0:1].clamp(-1, 1), utils.ScreenSpaceShading.normalize(rk[:, 1:4], dim=1), rk[:, 4:].clamp(0, 1)], dim=1)
        shade_cpu(prev)
        t_sr += time.perf_counter() - t0
        n_frames, last = n_frames + 1, qk
        cpu_frames.append((V.orbit_camera(k), gk, prev))
    # The same frames on the GPU.  Three passes over the sample, all outside the timed region:
    #  * free-running (what a viewer sees): frame k's "previous" is the GPU's own frame k - 1.  G-buffer parity holds per frame; the
    #    network output of frame k > 0 inherits frame k - 1's rounding differences through the recurrence, amplified by the
    #    network's gain (random-init weights: > 1) -- reported per frame as it is, NOT the kernels' parity figure;
    #  * TEACHER-FORCED single step (the kernels' parity claim, independent of the network's gain): frame k's "previous" is the CPU
    #    path's frame k - 1 output, uploaded -- every frame must be within 1e-4 of the CPU path's frame k;
    #  * both again on the exact-fp32 HIP kernels (ops.SPLIT_F16 = False): does the split-operand path behave like IEEE fp32 here?
    # (SuperresolutionNetwork/inference/loadedmodel.py:86-96 is the recurrence, mainComparisonVideo3.py:461-467 its driver.)
    from isosurfacesuperresolution_amd import ops

    def gpu_pass(teacher_forced):
        pipe.reset()
        out = []
        for k, (cam, g_cpu, raw_cpu) in enumerate(cpu_frames):
            if teacher_forced and k > 0:
                pipe.previous = cpu_frames[k - 1][2].to("cuda").contiguous()
            rgb_k, raw_k = pipe.frame(cam)
            torch.cuda.synchronize()
            out.append((rgb_k.clone() if k == 0 else None, raw_k.clone(), pipe.gbuffer.cpu().numpy()))
        return out

    def raw_err(frames):
        return [float((f[1].cpu() - c[2]).abs().max().item()) for f, c in zip(frames, cpu_frames)]

    free = gpu_pass(False)
    forced = gpu_pass(True)
    split_was = ops.SPLIT_F16
    ops.SPLIT_F16 = False
    try:
        exact_free, exact_forced = raw_err(gpu_pass(False)), raw_err(gpu_pass(True))
    finally:
        ops.SPLIT_F16 = split_was
        pipe.reset()
    err_free, err_forced = raw_err(free), raw_err(forced)
    rgb_gpu, raw_gpu, gbuf = free[0][0], free[0][1], free[0][2]
    # The CONDITIONING of each step, next to its error: the very step the CPU fp32 path took -- its G-buffer, its
    # previous frame -- evaluated in fp64 on the CPU; |CPU32 - that| is how far fp32 arithmetic alone puts the reference from the exact
    # result of the step through this (random-init) network.  A single-step error of the order of this figure is rounding, not a kernel.
    with contextlib.redirect_stdout(sys.stderr):
        net64 = models.createNetwork('EnhanceNet', 4, 101, [0, 1, 2, 3, 4], 6, opt)
    net64.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
    model64 = LoadedModel.from_model(net64.double().eval(), "cpu", parameters={"initialImage": "zero"})
    cond = []
    for k, (cam, g_cpu, raw_cpu) in enumerate(cpu_frames):
        r64 = model64.inference(torch.from_numpy(g_cpu).permute(2, 0, 1).unsqueeze(0).double(), cpu_frames[k - 1][2].double() if k > 0 else None)
        r64 = torch.cat([r64[:, 0:1].clamp(-1, 1), utils.ScreenSpaceShading.normalize(r64[:, 1:4], dim=1), r64[:, 4:].clamp(0, 1)], dim=1)
        cond.append(float((raw_cpu.double() - r64).abs().max().item()))
    per_frame = []
    for k, (cam, g_cpu, raw_cpu) in enumerate(cpu_frames):
        g_gpu = free[k][2]
        cols = [c for c in range(12) if k > 0 or c not in (8, 9)]       # the first frame's flow depends on the camera rendered before it
        per_frame.append({"mask_mismatches": int((g_gpu[..., 3] != g_cpu[..., 3]).sum()),
                          "gbuffer_max_abs_err": float(np.abs(g_gpu[..., cols] - g_cpu[..., cols]).max()),
                          "sr_raw_err_single_step": err_forced[k],            # teacher-forced: the kernels' claim (<= 1e-4)
                          "cpu32_vs_fp64_single_step": cond[k],               # the CPU fp32 reference's own distance from an fp64 evaluation of the same step
                          "sr_raw_err_free_running": err_free[k],             # the GPU's own recurrence (carries the network's gain)
                          "sr_raw_err_single_step_exact_f32": exact_forced[k],
                          "sr_raw_err_free_running_exact_f32": exact_free[k]})
    mse = torch.mean((rgb_gpu.cpu() - rgb_cpu) ** 2).item()
    psnr = 10 * np.log10(1 / max(1e-10, mse))      # mainVideoUnshaded.py:693
    bytes_alg = stats["bricks_touched"] * 2048 + low_w * low_h * 48
    out = {
        "cpu_baseline": {"value": n_frames / (t_render + t_sr), "unit": "frames/s", "cores": cores, "kind": "port",
                         "sample": "%d frames of the bench sequence: oracle ray-march %dx%d (%.3f s, OpenMP %d threads) + PyTorch CPU flow fill, warp, EnhanceNet, shading (%.3f s, %d threads)" % (
                             n_frames, low_w, low_h, t_render, cores, t_sr, cores)},
        "parity": {"frames_compared": len(per_frame),
                   "mask_mismatches": int(sum(f["mask_mismatches"] for f in per_frame)),                      # over ALL frames of the sample
                   "gbuffer_max_abs_err_excl_flow": float(np.abs(np.delete(gbuf, [8, 9], axis=2) - np.delete(ref, [8, 9], axis=2)).max()),
                   "gbuffer_max_abs_err": max(f["gbuffer_max_abs_err"] for f in per_frame),
                   # the kernels' parity figure: max over the frames of the TEACHER-FORCED single-step error (frame k computed from the
                   # CPU path's frame k - 1); tolerance 1e-4 (BASELINE.json north_star)
                   "sr_raw_max_abs_err": max(err_forced),
                   "sr_raw_max_abs_err_single_step": max(err_forced),        # the same figure under the name that says what it is
                   "schema_note": "since round 5 `sr_raw_max_abs_err` is the TEACHER-FORCED single-step maximum over the sample's frames (rounds "
                                  "<= 4: frame 0 of the GPU's own sequence = `sr_raw_max_abs_err_first_frame`); the free-running figures and "
                                  "their flags are separate keys",
                   "cpu32_vs_fp64_single_step_max": max(cond),
                   "sr_raw_max_abs_err_first_frame": err_forced[0],
                   "sr_raw_max_abs_err_free_running": max(err_free),
                   "sr_raw_max_abs_err_exact_f32": max(exact_forced),
                   "sr_raw_max_abs_err_free_running_exact_f32": max(exact_free),
                   "tolerance": 1e-4, "within_tolerance": bool(max(err_forced) <= 1e-4),
                   # the recurrent path has flags of its own: the plain tolerance (this random-init network amplifies rounding from frame to
                   # frame, so this one may read false on a correct path), and the bound a regression of the recurrence would break --
                   # the split-operand path grows no faster than the exact-fp32 HIP path does on the same frames
                   "within_tolerance_free_running": bool(max(err_free) <= 1e-4),
                   "free_running_within_2x_exact_f32": bool(max(err_free) <= 2.0 * max(exact_free) + 2e-6),
                   "psnr_rgb_vs_cpu_db": float(psnr),
                   "note": "single_step = frame k from the CPU path's frame k-1 (isolates the kernels); free_running = the GPU's own "
                           "recurrence, which also carries the random-init network's amplification of rounding differences from frame "
                           "to frame (the exact-fp32 HIP kernels show the same growth: *_exact_f32; tests/test_recurrence_gpu.py bounds "
                           "both against an fp64 CPU pass)",
                   "per_frame": per_frame},
    }
    result["raymarch"].update({
        "bricks_touched": stats["bricks_touched"], "samples": stats["samples"], "hit_pixels": stats["hits"],
        "algorithmic_bytes": bytes_alg, "achieved_GBps": bytes_alg / rm_time / 1e9,
        "frac_of_8TBps": bytes_alg / rm_time / 1e9 / HBM_PEAK_GBS, "samples_per_s": stats["samples"] / rm_time})
    return out


if __name__ == "__main__":
    main()
