"""Training-clip generator on the HIP renderer: clips are born on the device and can stay there.

Restates the reference's ``DataGenerator/DataGeneratorVideo2.py`` -- random camera paths and materials (``:135-151``), one
``GPURenderer.exe --animation`` run per clip (``GPURenderer/GPURenderer.cpp:807-856``: ``renderAnimation``), ``convertToNumpy``
(``:46-90``) -- on this package's ray-marcher, without the executable, the EXR files and the host round trips:

* ``random_clip_parameters`` draws what ``:135-151`` draw, from ONE ``numpy.random.RandomState``;
* ``clip_cameras`` interpolates the cameras as ``renderAnimation`` does, in fp32, and gives every frame the NEXT camera as its flow
  reference (``GPURenderer.cpp:811-829`` uploads it as ``nextViewMatrix``, ``render_kernel.cu:238-245``) -- for the last frame an
  extrapolated one;
* ``generate_clips`` renders every frame twice (low without AO, high with ``ao_samples`` world-space AO rays) into two reused
  G-buffers, fills the holes of the low flow (``ops.fill_flow_gbuffer``: this package's push-pull fill, ``inference/flowfill.py``,
  where the reference runs ``cv.inpaint(.., INPAINT_NS)``) and packs the frame into the flat clip buffers with ONE launch
  (``ops.pack_clip_frame``).  Nothing is read back;
* ``GeneratedClips`` hands the buffers to ``dataset_video.DeviceClips`` without a copy, samples crops from two small coverage tables
  per clip instead of the frames (``ops.clip_coverage``), and ``save`` writes the reference's ``.npy`` triples.

Renderer defaults are those of ``GPURenderer.cpp``'s ``Args`` (``:105-154``): field of view 45 (``:123``); the script passes
``--noshading 1`` (``:162``), ``--ao world`` with 256 samples of radius 1.0 (``:173-175``), a 512^2 image downscaled by 4.  ``--samples``
(``:167``) is parsed by the executable (``GPURenderer.cpp:236``) and never read by its renderer; it does not exist here.
``semantics="gvdb"`` (the default) is what ``GPURenderer.exe`` computes and what the released networks were trained on.

    python -m isosurfacesuperresolution_amd.datagen --descriptor inputs.dat --volumes DIR --out DIR [--clips 50 ...]
"""
import argparse
import collections
import os
import random

import numpy as np
import torch

from . import dataset_video, ops
from .dataset_video import MAX_AUGMENTATION_MODE, DeviceClips, Sample

FOV = 45.0                              # GPURenderer.cpp:123
OFFSET = (0.0, 0.0, -0.07)              # DataGeneratorVideo2.py:135-141: every origin and look-at is shifted by it
LOW_CHANNELS, HIGH_CHANNELS = len(ops.PACK_LOW_CHANNELS), len(ops.PACK_HIGH_CHANNELS)

ClipParameters = collections.namedtuple(
    "ClipParameters", "origin_start origin_end lookat_start lookat_end up isovalue diffuse specular exponent light raw")
ClipParameters.__doc__ = """What one clip is rendered with.  ``origin_*`` / ``lookat_*`` / ``up``: fp32 [3], the values the executable parses from the
script's ``%5.3f`` strings; ``isovalue``: float (the script passes ``str(isovalue)``); ``diffuse`` / ``specular`` / ``light``: the strings
themselves (``%5.3f`` triples, or ``'camera'``); ``exponent``: int; ``raw``: the unrounded draws (a dict of fp64 arrays: ``origin_start``,
``origin_end``, ``lookat_start``, ``lookat_end``, ``diffuse``, ``specular``, ``light`` or None)."""


def _fmt3(v):
    return "%5.3f,%5.3f,%5.3f" % (v[0], v[1], v[2])


def _parsed(v):
    """A vector after the ``%5.3f`` round trip, as the executable's fp32 ``Vector3DF``."""
    return np.array([np.float32(s) for s in _fmt3(v).split(",")], dtype=np.float32)


def _point_on_lower_hemisphere(rng):
    v = rng.randn(3)
    v /= np.linalg.norm(v)
    v[2] = -abs(v[2])
    return v


def random_clip_parameters(rng, min_iso, max_iso, max_dist=0.3):
    """The draws of ``DataGeneratorVideo2.py:135-151`` for one clip, from ``rng`` (a ``numpy.random.RandomState``; the reference mixes an
    unseeded ``np.random`` with ``random``), in this order:

    1. origin start: ``randn(3)`` (normalised, z = -|z|: the lower hemisphere), ``random_sample()`` for the radius in [0.6, 1.0);
    2. look-at start: ``randn(3)``, radius 0.1;
    3. origin end: ``randn(3)``, ``random_sample()`` -- both drawn AGAIN until ``|end - start| < max_dist``;
    4. look-at end: ``randn(3)``;
    5. isovalue: ``uniform(min_iso, max_iso)``;
    6. diffuse colour: ``uniform(0.2, 1.0, 3)``;
    7. specular colour: ``uniform(0, 1) ** 3 * 0.3``, three times the same;
    8. specular exponent: ``randint(4, 65)`` (4 .. 64);
    9. light: ``uniform(0, 1) < 0.7`` -> ``'camera'``, otherwise a direction: ``randn(3)`` as in 1.

    Every point is shifted by (0, 0, -0.07); up is (0, 0, -1).  The reference hands positions, colours and the light direction to the
    executable as ``%5.3f`` strings: the returned vectors have been through that formatting (``raw`` keeps the draws)."""
    offset = np.array(OFFSET)

    def origin():
        return _point_on_lower_hemisphere(rng) * (0.6 + rng.random_sample() * (1.0 - 0.6)) + offset
    origin_start = origin()
    lookat_start = _point_on_lower_hemisphere(rng) * 0.1 + offset
    while True:
        origin_end = origin()
        if np.linalg.norm(origin_end - origin_start) < max_dist:
            break
    lookat_end = _point_on_lower_hemisphere(rng) * 0.1 + offset
    isovalue = float(rng.uniform(min_iso, max_iso))
    diffuse = rng.uniform(0.2, 1.0, 3)
    specular = np.full(3, pow(rng.uniform(0, 1), 3) * 0.3)
    exponent = int(rng.randint(4, 65))
    direction = None if rng.uniform(0, 1) < 0.7 else _point_on_lower_hemisphere(rng)
    raw = dict(origin_start=origin_start, origin_end=origin_end, lookat_start=lookat_start, lookat_end=lookat_end, diffuse=diffuse,
               specular=specular, light=direction)
    return ClipParameters(_parsed(origin_start), _parsed(origin_end), _parsed(lookat_start), _parsed(lookat_end), _parsed((0, 0, -1)),
                          isovalue, _fmt3(diffuse), _fmt3(specular), exponent, "camera" if direction is None else _fmt3(direction), raw)


def _interpolate(a, b, alpha):
    # GPURenderer.cpp:803-806: Vector3DF(a) * (1 - alpha) + Vector3DF(b) * alpha with a float alpha
    alpha = np.float32(alpha)
    return a * (np.float32(1) - alpha) + b * alpha


def clip_cameras(params, frames):
    """``renderAnimation`` (``GPURenderer.cpp:807-823``): per frame j ``(origin, look-at, next origin, next look-at)``, fp32 [3] each.
    Frame j stands at ``alpha = j / (frames - 1)`` (divided in double, narrowed to float, then fp32 arithmetic as ``Vector3DF``'s); its
    flow reference at ``(j + 1) / (frames - 1)`` -- for the last frame that is past the end of the path: an extrapolated camera, not
    "no flow" as the executable's help text has it."""
    if frames < 2:
        raise ValueError("clip_cameras: an animation has at least two frames, got %d" % frames)
    out = []
    for j in range(frames):
        a, b = j / float(frames - 1), (j + 1) / float(frames - 1)
        out.append((_interpolate(params.origin_start, params.origin_end, a), _interpolate(params.lookat_start, params.lookat_end, a),
                    _interpolate(params.origin_start, params.origin_end, b), _interpolate(params.lookat_start, params.lookat_end, b)))
    return out


def _exact3(v):
    """fp32 [3] as a string whose numbers parse (as doubles) to exactly these values."""
    return "%.17g,%.17g,%.17g" % (float(v[0]), float(v[1]), float(v[2]))


def clip_commands(params, ao_radius, semantics):
    """The ``(command, value)`` strings of one clip that do not change from frame to frame."""
    return (("semantics", semantics), ("cameraFoV", "%g" % FOV), ("cameraUp", _fmt3(params.up)), ("isovalue", str(params.isovalue)),
            ("unshaded", "1"), ("diffuse", params.diffuse), ("specular", params.specular), ("exponent", str(params.exponent)),
            ("light", params.light), ("aoradius", str(float(ao_radius))))


def frame_commands(origin, lookat, resolution, ao_samples):
    """... and those of one render of one frame: the camera (fp32 values, written so that they parse back exactly), the image, the AO."""
    w, h = resolution
    return (("cameraOrigin", _exact3(origin)), ("cameraLookAt", _exact3(lookat)), ("resolution", "%d,%d" % (w, h)),
            ("viewport", "0,0,%d,%d" % (w, h)), ("aosamples", "%d" % ao_samples))


def _send(renderer, commands):
    for command, value in commands:
        if renderer.send_command(command, value) != 0:
            raise RuntimeError("datagen: the renderer refused %s=%s" % (command, value))


def render_frame(renderer, camera, low_gbuf, high_gbuf, ao_samples):
    """The two renders of one frame (``renderAnimation``'s high and low pass) into ``high_gbuf`` [H, W, 12] and ``low_gbuf`` [h, w, 12].
    Each is measured against the NEXT camera: a render leaves its own camera behind as the flow reference, so the next one is set
    before both.  The low pass runs without AO (the reference renders it with the same AO setting, and never saves that channel)."""
    origin, lookat, next_origin, next_lookat = camera
    for gbuf, ao in ((low_gbuf, 0), (high_gbuf, ao_samples)):
        renderer.set_last_camera(next_origin, next_lookat)
        _send(renderer, frame_commands(origin, lookat, (gbuf.shape[1], gbuf.shape[0]), ao))
        if renderer.render_direct(gbuf) < 0:
            raise RuntimeError("datagen: the render failed")


def _filled_flow(low_gbuf):
    if low_gbuf.is_cuda:
        return ops.fill_flow_gbuffer(low_gbuf)
    from .inference.flowfill import fill_flow
    planes = low_gbuf.permute(2, 0, 1)
    return fill_flow(planes[8:10].unsqueeze(0), planes[3:4].unsqueeze(0) != 0)


def _clip_rows(sizes, frames, upscale):
    """Clip table rows ``(high offset, low offset, flow offset, H, W)`` of clips of the low-resolution ``sizes`` laid out one after the
    other, every clip starting on a multiple of four elements of ``high`` (``DeviceClips``' layout), and the three buffer lengths."""
    rows, off = [], [0, 0, 0]
    for H, W in sizes:
        rows.append((off[0], off[1], off[2], H, W))
        off[0] += -(-(frames * HIGH_CHANNELS * upscale * H * upscale * W) // 4) * 4
        off[1] += frames * LOW_CHANNELS * H * W
        off[2] += frames * 2 * H * W
    return rows, off


class GeneratedClips:
    """Clips in three flat fp32 buffers ``high`` / ``low`` / ``flow`` on one device -- clip k is ``[T, 6, r H, r W]``, ``[T, 5, H, W]`` and
    ``[T, 2, H, W]`` behind the offsets of ``rows[k] = (high, low, flow offset, H, W)`` (``table``: the same as int64 [clips, 5] on the
    device, ``DeviceClips``' format) -- and the ``parameters`` each was rendered with."""

    def __init__(self, high, low, flow, rows, frames, upscale, parameters=None):
        self.high, self.low, self.flow = high, low, flow
        self.rows = [tuple(int(v) for v in row) for row in rows]
        self.frames, self.upscale = int(frames), int(upscale)
        self.low_channels, self.high_channels = LOW_CHANNELS, HIGH_CHANNELS
        self.parameters = list(parameters) if parameters is not None else [None] * len(self.rows)
        self.device = high.device
        self.table = torch.tensor(self.rows, dtype=torch.int64).reshape(-1, 5).to(self.device)
        self._coverage = None

    @classmethod
    def from_arrays(cls, clips, device="cpu"):
        """From ``(high, low, flow)`` numpy triples in the reference's shapes (clips may differ in size)."""
        frames = int(clips[0][1].shape[0])
        upscale = int(clips[0][0].shape[2]) // int(clips[0][1].shape[2])
        rows, sizes = _clip_rows([tuple(low.shape[2:]) for _, low, _ in clips], frames, upscale)
        buffers = [torch.zeros(n, dtype=torch.float32, device=device) for n in sizes]
        for row, arrays in zip(rows, clips):
            for buf, start, a in zip(buffers, row, arrays):
                buf[start:start + a.size].copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).reshape(-1))
        return cls(buffers[0], buffers[1], buffers[2], rows, frames, upscale)

    def __len__(self):
        return len(self.rows)

    def clip(self, k):
        """Views ``(high [T, 6, r H, r W], low [T, 5, H, W], flow [T, 2, H, W])`` of clip k."""
        oh, ol, of, H, W = self.rows[k]
        T, r = self.frames, self.upscale
        return (self.high[oh:oh + T * HIGH_CHANNELS * r * H * r * W].view(T, HIGH_CHANNELS, r * H, r * W),
                self.low[ol:ol + T * LOW_CHANNELS * H * W].view(T, LOW_CHANNELS, H, W), self.flow[of:of + T * 2 * H * W].view(T, 2, H, W))

    def coverage_tables(self):
        """Per clip an int32 numpy array ``[2, H + 1, W + 1]``: the summed-area tables of the coverage indicator of frames 0 and T - 1
        (``ops.clip_coverage``: one launch), downloaded once -- the only thing ``collect_samples`` needs from the device."""
        if self._coverage is None:
            flat = ops.clip_coverage(self.low, self.table, self.frames, LOW_CHANNELS, rows=self.rows).reshape(-1).cpu().numpy()
            offsets, _ = ops.coverage_table_offsets(self.rows)
            self._coverage = [flat[o:o + 2 * (H + 1) * (W + 1)].reshape(2, H + 1, W + 1) for o, (_, _, _, H, W) in zip(offsets, self.rows)]
        return self._coverage

    def collect_samples(self, num_samples, seed=None, crop=dataset_video.CROP):
        """``dataset_video.collect_samples`` without the frames: the same ``random.Random(seed)`` calls in the same order (``randint`` for
        the clip, the row, the column; ``randrange`` for the augmentation mode of an accepted crop only), the coverage of a candidate
        from four look-ups in each of the two tables.  Returns the sorted list of ``Sample`` -- element for element what
        ``dataset_video.collect_samples(saved_folder, num_samples, seed=seed, crop=crop).samples`` is."""
        tables = self.coverage_tables()
        rng = random.Random(seed)
        fill = 0.5 * crop * crop
        r = self.upscale

        def acceptable(sat, H, W):                       # is there a crop position (of those randint can draw) that passes?
            sat = sat.astype(np.int64)
            counts = sat[:, crop:, crop:] - sat[:, :-crop, crop:] - sat[:, crop:, :-crop] + sat[:, :-crop, :-crop]
            return bool(((counts[0] >= fill) & (counts[1] >= fill))[:H - crop, :W - crop].any())
        if crop < 1 or not any(acceptable(t, row[3], row[4]) for t, row in zip(tables, self.rows)):
            raise ValueError("GeneratedClips.collect_samples: no %d x %d crop of any clip is half covered in its first and last frame "
                             "(the reference's loop would not end)" % (crop, crop))
        samples = []
        while len(samples) < num_samples:
            idx = rng.randint(0, len(self.rows) - 1)
            H, W = self.rows[idx][3:]
            x = rng.randint(0, H - crop - 1)
            y = rng.randint(0, W - crop - 1)
            sat = tables[idx]
            covered = sat[:, x + crop, y + crop].astype(np.int64) - sat[:, x, y + crop] - sat[:, x + crop, y] + sat[:, x, y]
            if covered[0] >= fill and covered[1] >= fill:
                samples.append(Sample(idx, (x, x + crop, y, y + crop), (r * x, r * (x + crop), r * y, r * (y + crop)),
                                      rng.randrange(MAX_AUGMENTATION_MODE)))
        samples.sort(key=lambda s: s.index)
        return samples

    def device_clips(self, samples):
        """A ``DeviceClips`` over THESE buffers (no copy) with the sample list ``samples``: what ``DeviceBatchLoader`` and ``train.fit``
        take."""
        if not samples:
            raise ValueError("GeneratedClips.device_clips: no samples")
        crop = int(samples[0].crop_low[1]) - int(samples[0].crop_low[0])
        return DeviceClips.from_buffers(self.high, self.low, self.flow, self.rows, samples, self.frames, LOW_CHANNELS, HIGH_CHANNELS, crop,
                                        self.upscale)

    def save(self, folder):
        """``high_%05d.npy`` / ``low_%05d.npy`` / ``flow_%05d.npy`` in the reference's shapes: what ``dataset_video.collect_samples`` and the
        reference's trainer read."""
        os.makedirs(folder, exist_ok=True)
        for k in range(len(self.rows)):
            for name, t in zip(("high", "low", "flow"), self.clip(k)):
                np.save(os.path.join(folder, "%s_%05d.npy" % (name, k)), t.cpu().numpy())


def generate_clips(renderer, num_clips, frames=10, high_res=512, downscale=4, ao_samples=256, ao_radius=1.0, iso_range=(0.1, 0.5), seed=None,
                   device="cuda", semantics="gvdb"):
    """``num_clips`` clips of ``frames`` frames of the volume loaded into ``renderer`` (a ``DirectRenderer``), with the reference's
    defaults: 512^2 high-resolution frames with 256 world-space AO rays of radius 1.0, low-resolution frames a quarter of that, random
    paths and materials (``random_clip_parameters`` from ``RandomState(seed)``; isovalue in ``iso_range``).  Per frame: two renders into
    two reused G-buffers, the flow fill of the low one, ONE ``ops.pack_clip_frame`` launch that writes the frame's planes into the flat
    buffers at the clip's offsets -- nothing is read back.  Returns ``GeneratedClips`` on ``device``."""
    if semantics not in ("gvdb", "cpu"):
        raise ValueError("generate_clips: semantics is 'gvdb' or 'cpu', got %r" % (semantics,))
    if num_clips < 1 or frames < 2 or downscale < 1 or high_res < downscale or high_res % downscale:
        raise ValueError("generate_clips: %d clips of %d frames at %d / %d" % (num_clips, frames, high_res, downscale))
    low_res = high_res // downscale
    rng = np.random.RandomState(seed)
    rows, sizes = _clip_rows([(low_res, low_res)] * num_clips, frames, downscale)
    high, low, flow = (torch.zeros(n, dtype=torch.float32, device=device) for n in sizes)
    low_gbuf = torch.empty((low_res, low_res, 12), dtype=torch.float32, device=device)
    high_gbuf = torch.empty((high_res, high_res, 12), dtype=torch.float32, device=device)
    n = low_res * low_res
    parameters = []
    for off_high, off_low, off_flow, _, _ in rows:
        params = random_clip_parameters(rng, iso_range[0], iso_range[1])
        parameters.append(params)
        _send(renderer, clip_commands(params, ao_radius, semantics))
        for j, camera in enumerate(clip_cameras(params, frames)):
            render_frame(renderer, camera, low_gbuf, high_gbuf, ao_samples)
            ops.pack_clip_frame(low_gbuf, high_gbuf, _filled_flow(low_gbuf), high, low, flow,
                                (off_high + j * HIGH_CHANNELS * downscale * downscale * n, off_low + j * LOW_CHANNELS * n, off_flow + j * 2 * n))
    return GeneratedClips(high, low, flow, rows, frames, downscale, parameters)


def read_descriptor(path):
    """The reference's ``inputs.dat`` (``DataGeneratorVideo2.py:99-107``): one header line, then ``name min_iso max_iso`` per line.
    Returns ``[(name, min_iso, max_iso)]``."""
    out = []
    with open(path) as f:
        lines = f.read().splitlines()[1:]
    for number, line in enumerate(lines, 2):
        fields = line.split()
        if not fields:
            continue
        if len(fields) != 3:
            raise ValueError("%s:%d: expected 'name min_iso max_iso', got %r" % (path, number, line))
        out.append((fields[0], float(fields[1]), float(fields[2])))
    if not out:
        raise ValueError("%s: no volumes listed" % path)
    return out


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m isosurfacesuperresolution_amd.datagen",
                                description="Training clips (high / low / flow .npy triples) of the volumes of a descriptor file.")
    p.add_argument("--descriptor", required=True, help="the reference's inputs.dat: a header line, then 'name min_iso max_iso' per line")
    p.add_argument("--volumes", required=True, help="folder of the .vbx volumes the descriptor names")
    p.add_argument("--out", required=True, help="output folder: one sub-folder per volume and clips.txt listing them")
    p.add_argument("--clips", type=int, default=50, help="clips per volume (numImages)")
    p.add_argument("--frames", type=int, default=10)
    p.add_argument("--high", type=int, default=512, help="edge of the high-resolution frames")
    p.add_argument("--downscale", type=int, default=4)
    p.add_argument("--aosamples", type=int, default=256)
    p.add_argument("--aoradius", type=float, default=1.0)
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--semantics", choices=("gvdb", "cpu"), default="gvdb")
    return p.parse_args(argv)


def main(argv=None):
    from .inference import DirectRenderer
    args = parse_args(argv)
    volumes = read_descriptor(args.descriptor)
    os.makedirs(args.out, exist_ok=True)
    renderer = DirectRenderer()
    folders = []
    for k, (name, min_iso, max_iso) in enumerate(volumes):
        if renderer.load(os.path.join(args.volumes, name)) != 0:
            raise RuntimeError("datagen: cannot load %s" % os.path.join(args.volumes, name))
        clips = generate_clips(renderer, args.clips, args.frames, args.high, args.downscale, args.aosamples, args.aoradius, (min_iso, max_iso),
                               None if args.seed is None else args.seed + k, "cuda", args.semantics)
        folders.append(os.path.splitext(name)[0])
        clips.save(os.path.join(args.out, folders[-1]))
        print("%s: %d clips of %d frames, iso in [%g, %g]" % (name, args.clips, args.frames, min_iso, max_iso))
    with open(os.path.join(args.out, "clips.txt"), "w") as f:
        f.write("".join(folder + "\n" for folder in folders))


if __name__ == "__main__":
    main()
