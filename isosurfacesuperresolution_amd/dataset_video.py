"""Training-clip dataset of the unshaded pipeline (data contract of SURVEY.md S11).

Restates the array branch of ``SuperresolutionNetwork/datasetVideo.py`` (``collect_samples_clouds_video``
``:84-309`` with ``load_arrays``; ``DatasetFromSamples`` ``:311-366``):

* clips are triples ``high_%05d.npy [T,6,4H,4W]``, ``low_%05d.npy [T,5,H,W]`` (mask in [-1,1], normal,
  depth), ``flow_%05d.npy [T,2,H,W]`` (hole-filled), consecutively numbered in a folder, or in the
  sub-folders listed line by line in a text file;
* a sample is a random 32^2 low-res crop (128^2 high-res) whose first AND last frame are at least
  50 % covered (``:267-283``: coverage = pixels where the sum of the first three low-res channels > 0);
* samples are sorted by clip index and the LAST ``test_fraction`` of them form the test set
  (``:300-301,328-334``) so that train and test never share a clip region ordering;
* optional flip augmentation with the sign fix-ups of ``:31-78`` (off by default as in the reference).

``DatasetFromSamples`` under a ``DataLoader`` is the reference's host path.  ``DeviceClips`` + ``DeviceBatchLoader`` keep the clips
on the device and make a batch one gather launch (``ops.gather_clips``), with the same split, order and bits.
"""
import os
import random
from collections import namedtuple

import numpy as np
import torch
from torch.utils import data

CROP = 32
MAX_AUGMENTATION_MODE = 4
Sample = namedtuple("Sample", "index crop_low crop_high augmentation")
DatasetData = namedtuple("DatasetData", "samples images_high images_low flow_low input_channels output_channels crop_size num_frames")


def _clip_paths(path):
    def names(folder, i):
        return tuple(os.path.join(folder, "%s_%05d.npy" % (m, i)) for m in ("high", "low", "flow"))
    folders = [path]
    if os.path.isfile(path):
        with open(path) as f:
            folders = [os.path.join(os.path.dirname(path), line.strip()) for line in f if line.strip()]
    out = []
    for folder in folders:
        i = 0
        while os.path.exists(names(folder, i)[1]):
            out.append(names(folder, i))
            i += 1
    return out


def data_augmentation(low, high, flow, mode, enabled=False):
    if not enabled:
        return low, high, flow
    flip_x, flip_y = bool(mode & 1), bool(mode & 2)
    axes = tuple(a for a, f in ((2, flip_x), (3, flip_y)) if f)
    if not axes:
        return low, high, flow
    low, high, flow = (np.flip(t, axis=axes).copy() for t in (low, high, flow))
    if low.shape[1] in (7, 8):                      # shaded layouts carry a normal at channels 4,5
        if flip_x: low[:, 4] = -low[:, 4]
        if flip_y: low[:, 5] = -low[:, 5]
    if flip_x: flow[:, 0] = -flow[:, 0]
    if flip_y: flow[:, 1] = -flow[:, 1]
    return low, high, flow


def collect_samples(path, num_samples, upsampling=4, number_of_images=None, seed=None, crop=CROP):
    paths = _clip_paths(path)
    if not paths:
        raise ValueError("No image found")
    if number_of_images:
        paths = paths[:number_of_images]
    high = [np.load(p[0]) for p in paths]
    low = [np.load(p[1]) for p in paths]
    flow = [np.load(p[2]) for p in paths]
    T = low[0].shape[0]
    rng = random.Random(seed)
    fill = 0.5 * crop * crop
    samples = []
    while len(samples) < num_samples:
        idx = rng.randint(0, len(paths) - 1)
        d2, d3 = low[idx].shape[2], low[idx].shape[3]
        x = rng.randint(0, d2 - crop - 1)
        y = rng.randint(0, d3 - crop - 1)
        def covered(t):
            c = low[idx][t, 0:3, x:x + crop, y:y + crop].sum(axis=0) > 0
            return c.sum() >= fill
        if covered(0) and covered(T - 1):
            samples.append(Sample(idx, (x, x + crop, y, y + crop),
                                  (upsampling * x, upsampling * (x + crop), upsampling * y, upsampling * (y + crop)),
                                  rng.randrange(MAX_AUGMENTATION_MODE)))
    samples.sort(key=lambda s: s.index)
    return DatasetData(samples, high, low, flow, 5, high[0].shape[1], crop, T)


class DatasetFromSamples(data.Dataset):
    """``__getitem__`` -> (low [T,5,c,c], flow [T,2,c,c], high [T,6,4c,4c])"""

    def __init__(self, dataset_data, test, test_fraction, augmentation=False):
        self.data = dataset_data
        self.samples = dataset_data.samples
        n = len(self.samples)
        l = int(n * test_fraction)
        self.index_offset, self.num_images = (n - l, l) if test else (0, n - l)
        self.augmentation = augmentation

    def __len__(self):
        return self.num_images

    def __getitem__(self, index):
        s = self.samples[index + self.index_offset]
        cl, ch = s.crop_low, s.crop_high
        low = self.data.images_low[s.index][:, :, cl[0]:cl[1], cl[2]:cl[3]]
        flow = self.data.flow_low[s.index][:, :, cl[0]:cl[1], cl[2]:cl[3]]
        high = self.data.images_high[s.index][:, :, ch[0]:ch[1], ch[2]:ch[3]]
        low, high, flow = data_augmentation(low, high, flow, s.augmentation, self.augmentation)
        return (torch.from_numpy(np.ascontiguousarray(low)), torch.from_numpy(np.ascontiguousarray(flow)),
                torch.from_numpy(np.ascontiguousarray(high)))


def _sample_table(samples, rows, c, r):
    """The int32 [n, 4] sample table of ``DeviceClips`` as a list, every sample checked against the clip rows ``(.., .., .., H, W)``."""
    table = []
    for j, s in enumerate(samples):
        x0, x1, y0, y1 = (int(v) for v in s.crop_low)
        if not 0 <= s.index < len(rows):
            raise ValueError("DeviceClips: sample %d: clip %d of %d" % (j, s.index, len(rows)))
        H, W = rows[s.index][3:]
        if x1 - x0 != c or y1 - y0 != c or x0 < 0 or y0 < 0 or x1 > H or y1 > W:
            raise ValueError("DeviceClips: sample %d: the crop rows %d:%d, columns %d:%d is not a %d x %d box inside clip %d (%d x %d)"
                             % (j, x0, x1, y0, y1, c, c, s.index, H, W))
        if tuple(int(v) for v in s.crop_high) != (r * x0, r * x1, r * y0, r * y1):
            raise ValueError("DeviceClips: sample %d: the high-resolution box %s is not %d times the low-resolution one" % (j, tuple(s.crop_high), r))
        if not 0 <= int(s.augmentation) < MAX_AUGMENTATION_MODE:
            raise ValueError("DeviceClips: sample %d: augmentation mode %d" % (j, s.augmentation))
        table.append((s.index, x0, y0, int(s.augmentation)))
    if not table:
        raise ValueError("DeviceClips: no samples")
    return table


class DeviceClips:
    """A ``DatasetData`` resident on ``device``: every clip uploaded ONCE, clip by clip, into three flat fp32 buffers (``high``, ``low``,
    ``flow``), plus the two tables ``ops.gather_clips`` reads -- ``table`` int64 [clips, 5] (element offset of the clip in each buffer,
    low-resolution height and width; clips may differ in size) and ``samples`` int32 [n, 4] (clip, first row, first column of the
    low-resolution crop, augmentation mode), in the order of ``dataset_data.samples``.  A batch is then one launch
    (``DeviceBatchLoader``).  Everything the kernel relies on is checked here, on the host: a clip that is not fp32 and a sample whose
    box leaves its clip raise ``ValueError``; a set that does not fit in the device's free memory is refused with the byte counts.
    ``device="cpu"`` holds CPU tensors: the same objects run everywhere.  ``nbytes``: what the buffers and tables take."""

    def __init__(self, dataset_data, device="cuda"):
        dd = dataset_data
        self.device = torch.device(device)
        if not dd.images_low:
            raise ValueError("DeviceClips: no clips")
        self.frames, self.low_channels = int(dd.images_low[0].shape[0]), int(dd.images_low[0].shape[1])
        self.high_channels = int(dd.images_high[0].shape[1])
        self.crop = int(dd.crop_size)
        self.upscale = int(dd.images_high[0].shape[2]) // int(dd.images_low[0].shape[2])
        T, Cl, Ch, r, c = self.frames, self.low_channels, self.high_channels, self.upscale, self.crop
        rows, off = [], [0, 0, 0]
        for i, (high, low, flow) in enumerate(zip(dd.images_high, dd.images_low, dd.flow_low)):
            for name, a in (("high", high), ("low", low), ("flow", flow)):
                if a.dtype != np.float32:
                    raise ValueError("DeviceClips: clip %d: %s is %s, not float32" % (i, name, a.dtype))
            H, W = int(low.shape[2]), int(low.shape[3])
            if low.shape != (T, Cl, H, W) or flow.shape != (T, 2, H, W) or high.shape != (T, Ch, r * H, r * W) or r < 1:
                raise ValueError("DeviceClips: clip %d: shapes high %s, low %s, flow %s are not [%d, %d, %d H, %d W], [%d, %d, H, W], [%d, 2, H, W]"
                                 % (i, high.shape, low.shape, flow.shape, T, Ch, r, r, T, Cl, T))
            rows.append((off[0], off[1], off[2], H, W))
            off[0] += -(-high.size // 4) * 4              # every clip starts on a multiple of four elements: 16-byte rows for the gather
            off[1] += low.size
            off[2] += flow.size
        table = _sample_table(dd.samples, rows, c, r)
        self.nbytes = 4 * sum(off) + 8 * 5 * len(rows) + 4 * 4 * len(table)
        if self.device.type == "cuda":
            free, total = torch.cuda.mem_get_info(self.device)
            if self.nbytes > free:
                raise RuntimeError("DeviceClips: the clips take %d bytes (high %d, low %d, flow %d); %s has %d of %d bytes free"
                                   % (self.nbytes, 4 * off[0], 4 * off[1], 4 * off[2], self.device, free, total))
        self.high, self.low, self.flow = (torch.empty(n, dtype=torch.float32, device=self.device) for n in off)
        for row, arrays in zip(rows, zip(dd.images_high, dd.images_low, dd.flow_low)):
            for buf, start, a in zip((self.high, self.low, self.flow), row, arrays):
                buf[start:start + a.size].copy_(torch.from_numpy(np.ascontiguousarray(a)).reshape(-1))
        self.high_quad_aligned = True
        self.table = torch.tensor(rows, dtype=torch.int64).to(self.device)
        self.samples = torch.tensor(table, dtype=torch.int32).to(self.device)
        self.num_samples, self.num_clips = len(table), len(rows)

    @classmethod
    def from_buffers(cls, high, low, flow, table_rows, samples, frames, low_channels, high_channels, crop, upscale):
        """ADOPT clips that already lie in flat fp32 buffers (``datagen.GeneratedClips``: rendered into them on the device) -- no copy.
        ``table_rows``: per clip ``(high offset, low offset, flow offset, H, W)``; ``samples``: a list of ``Sample``.  The same checks
        as the constructor's: fp32 buffers, clips inside them, every sample's box inside its clip."""
        self = cls.__new__(cls)
        buffers = (high, low, flow)
        for name, t in zip(("high", "low", "flow"), buffers):
            if t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous():
                raise ValueError("DeviceClips: %s is %s %s, not a flat float32 buffer" % (name, t.dtype, tuple(t.shape)))
        if len({t.device for t in buffers}) != 1:
            raise ValueError("DeviceClips: buffers on more than one device")
        rows = [tuple(int(v) for v in row) for row in table_rows]
        if not rows:
            raise ValueError("DeviceClips: no clips")
        T, Cl, Ch, r, c = int(frames), int(low_channels), int(high_channels), int(upscale), int(crop)
        for i, row in enumerate(rows):
            H, W = (row[3], row[4]) if len(row) == 5 else (0, 0)
            sizes = (T * Ch * r * H * r * W, T * Cl * H * W, T * 2 * H * W)
            if H < 1 or W < 1 or r < 1 or T < 1 or any(not 0 <= off <= t.numel() - n for off, t, n in zip(row, buffers, sizes)):
                raise ValueError("DeviceClips: clip %d: row %s with %d frames, %d / %d channels, upscale %d leaves the buffers (%d, %d, %d elements)"
                                 % (i, row, T, Ch, Cl, r, high.numel(), low.numel(), flow.numel()))
        table = _sample_table(samples, rows, c, r)
        self.device = high.device
        self.frames, self.low_channels, self.high_channels, self.crop, self.upscale = T, Cl, Ch, c, r
        self.high, self.low, self.flow = buffers
        self.high_quad_aligned = all(row[0] % 4 == 0 for row in rows)
        self.table = torch.tensor(rows, dtype=torch.int64).to(self.device)
        self.samples = torch.tensor(table, dtype=torch.int32).to(self.device)
        self.num_samples, self.num_clips = len(table), len(rows)
        self.nbytes = 4 * (high.numel() + low.numel() + flow.numel()) + 8 * 5 * len(rows) + 4 * 4 * len(table)
        return self


class DeviceBatchLoader:
    """The training loops' fast path: an iterable (with ``__len__``) of ``(input, flow, target)`` batches on the device, each ONE launch
    of ``ops.gather_clips`` on a ``DeviceClips`` (a ``DatasetData`` is uploaded first) -- what ``DataLoader(DatasetFromSamples(...))``
    yields, bit for bit, without the host's slicing, collating and copying.

    Split: ``DatasetFromSamples``' -- the samples are sorted by clip and the last ``int(n * test_fraction)`` are the test set.  Order: an
    epoch is ``arange(n)``, or with ``shuffle`` ``torch.randperm(n, generator=g)`` of a CPU generator seeded with ``seed`` (successive
    epochs continue its stream); it is uploaded ONCE per epoch (``order`` keeps the host copy) and every batch's index vector is a slice
    of that device tensor: within an epoch nothing is copied to the device and nothing is ever read back.  A ragged last batch is
    yielded unless ``drop_last``.  Every batch is three fresh tensors: a consumer may keep it.  ``rank`` / ``world_size``: only this
    rank's slice of each global batch of ``batch_size`` is gathered -- ``DataParallelTrainer.shard(global_batch)``; every global batch
    must divide evenly."""

    def __init__(self, clips, batch_size, test=False, test_fraction=0.2, shuffle=False, augmentation=False, drop_last=False, seed=None,
                 device="cuda", rank=0, world_size=1):
        self.clips = clips if isinstance(clips, DeviceClips) else DeviceClips(clips, device)
        self.device = self.clips.device
        n = self.clips.num_samples
        held_out = int(n * test_fraction)
        self.index_offset, self.num_images = (n - held_out, held_out) if test else (0, n - held_out)
        self.batch_size, self.shuffle, self.augmentation, self.drop_last = int(batch_size), shuffle, augmentation, drop_last
        self.rank, self.world_size = int(rank), int(world_size)
        if self.batch_size < 1 or self.world_size < 1 or not 0 <= self.rank < self.world_size:
            raise ValueError("DeviceBatchLoader: batch_size %d, rank %d of %d" % (self.batch_size, self.rank, self.world_size))
        ragged = 0 if drop_last else self.num_images % self.batch_size
        if self.batch_size % self.world_size or ragged % self.world_size:
            raise ValueError("DeviceBatchLoader: global batches of %d%s samples do not divide evenly over %d ranks"
                             % (self.batch_size, " and %d" % ragged if ragged else "", self.world_size))
        self.generator = torch.Generator()
        if seed is None:
            self.generator.seed()
        else:
            self.generator.manual_seed(seed)
        self.order = None

    def __len__(self):
        return self.num_images // self.batch_size if self.drop_last else -(-self.num_images // self.batch_size)

    def __iter__(self):
        from . import ops
        n = self.num_images
        self.order = torch.randperm(n, generator=self.generator) if self.shuffle else torch.arange(n)
        order = (self.order + self.index_offset).to(self.device)               # the epoch's one upload
        for k in range(len(self)):
            lo = k * self.batch_size
            per = (min(n, lo + self.batch_size) - lo) // self.world_size
            indices = order[lo + self.rank * per:lo + (self.rank + 1) * per]
            yield ops.gather_clips(self.clips, self.clips.samples, indices, self.clips.crop, self.augmentation)


def render_clip(renderer, origins, low_res, upscale=4, fov=30.0, isovalue=0.34, ao_samples=0, ao_radius=0.05):
    """Produce one training clip with this package's renderer, in the format above
    (the reference drives GPURenderer.exe for this: ``DataGenerator/DataGeneratorVideo2.py:46-90``)."""
    from .inference.flowfill import fill_flow
    from .volumes import fmt3
    w, h = low_res
    r = renderer
    for c, v in (("cameraLookAt", "0,0,0"), ("cameraUp", "0,1,0"), ("cameraFoV", "%.3f" % fov), ("isovalue", "%5.3f" % isovalue),
                 ("aoradius", "%5.3f" % ao_radius)):
        r.send_command(c, v)
    lows, highs, flows = [], [], []
    for origin in origins:
        r.send_command("cameraOrigin", fmt3(origin))
        frames = {}
        for name, (W, H), ao in (("low", (w, h), 0), ("high", (w * upscale, h * upscale), ao_samples)):
            r.send_command("resolution", "%d,%d" % (W, H))
            r.send_command("viewport", "0,0,%d,%d" % (W, H))
            r.send_command("aosamples", "%d" % ao)
            if name == "high":          # keep the flow reference of the low-res stream: re-send the same camera
                pass
            buf = torch.empty((H, W, 12), dtype=torch.float32, device="cuda")
            r.render_direct(buf)
            frames[name] = buf.permute(2, 0, 1)
        lo, hi = frames["low"], frames["high"]
        lows.append(torch.cat((lo[3:4] * 2 - 1, lo[4:8]), 0))
        highs.append(torch.cat((hi[3:4] * 2 - 1, hi[4:8], hi[10:11]), 0))
        flows.append(fill_flow(lo[8:10].unsqueeze(0), lo[3:4].unsqueeze(0) != 0)[0])
    return (torch.stack(highs).cpu().numpy(), torch.stack(lows).cpu().numpy(), torch.stack(flows).cpu().numpy())
