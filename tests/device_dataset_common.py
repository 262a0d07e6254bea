"""What the tests of the device-resident training clips share (test_device_dataset_cpu.py, test_device_dataset_gpu.py): a small
``DatasetData`` generated from a seed, its batch index vector, and the host path's batch for it.

Three clips of DIFFERENT sizes -- low 20 x 28, 16 x 36 and 8 x 8 (with c = 8 the last crop IS the clip) -- of T = 3 frames, c = 8,
r = 4; low with 5 or 8 channels (8: a shaded layout, whose channels 4 and 5 change sign under the flips), high with 6.  Exact zeros are
planted in the flow and in low channels 4-5, so that a negation has to produce -0.0.  Per clip three crop positions -- (0, 0),
(H - c, W - c) and (1, 3) (both borders, an odd unaligned column; clipped to the clip where it does not fit: the 8 x 8 clip) -- each in
all four augmentation modes: 36 samples, sample = 12 clip + 4 position + mode.  The batch [5, 0, 35, 17, 17, 2, 30] is unsorted, has a
repeat and touches every clip."""
import numpy as np
import torch

SIZES = ((20, 28), (16, 36), (8, 8))
T, CROP, UPSCALE, HIGH_CHANNELS = 3, 8, 4, 6
BATCH = (5, 0, 35, 17, 17, 2, 30)


def random_clip(rng, frames, low_channels, high_channels, H, W, upscale):
    """(high, low, flow) of one clip: signed values, exact zeros in a tenth of the flow and of low channels 4-5."""
    low = rng.standard_normal((frames, low_channels, H, W)).astype(np.float32)
    flow = rng.standard_normal((frames, 2, H, W)).astype(np.float32)
    high = rng.standard_normal((frames, high_channels, upscale * H, upscale * W)).astype(np.float32)
    flow[rng.random(flow.shape) < 0.1] = 0.0
    if low_channels > 5:
        part = low[:, 4:6]
        part[rng.random(part.shape) < 0.1] = 0.0
    else:
        low[:, 4][rng.random(low[:, 4].shape) < 0.1] = 0.0
    return high, low, flow


def make_sample(D, clip, x0, y0, crop, upscale, mode):
    return D.Sample(clip, (x0, x0 + crop, y0, y0 + crop), tuple(upscale * v for v in (x0, x0 + crop, y0, y0 + crop)), mode)


def dataset(low_channels, seed=11):
    """The fixture as a ``dataset_video.DatasetData``."""
    from isosurfacesuperresolution_amd import dataset_video as D
    rng = np.random.default_rng(seed)
    highs, lows, flows, samples = [], [], [], []
    for k, (H, W) in enumerate(SIZES):
        high, low, flow = random_clip(rng, T, low_channels, HIGH_CHANNELS, H, W, UPSCALE)
        highs.append(high); lows.append(low); flows.append(flow)
        for x0, y0 in ((0, 0), (H - CROP, W - CROP), (min(1, H - CROP), min(3, W - CROP))):
            for mode in range(4):
                samples.append(make_sample(D, k, x0, y0, CROP, UPSCALE, mode))
    return D.DatasetData(samples, highs, lows, flows, low_channels, HIGH_CHANNELS, CROP, T)


def host_batch(dataset_data, indices, augmentation):
    """The host path for the samples ``indices``: ``DatasetFromSamples.__getitem__`` (with ``data_augmentation``) + the default collate."""
    from isosurfacesuperresolution_amd import dataset_video as D
    items = D.DatasetFromSamples(dataset_data, False, 0.0, augmentation)
    return tuple(torch.utils.data.default_collate([items[i] for i in indices]))


def same_bits(a, b):
    """Equal as int32 views: the sign of a zero counts."""
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.cpu().contiguous().view(torch.int32),
                                                                                      b.cpu().contiguous().view(torch.int32))


def negative_zeros(t):
    return int((t.cpu().contiguous().view(torch.int32) == -2 ** 31).sum())
