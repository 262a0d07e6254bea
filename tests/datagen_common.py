"""What the tests of the clip generator share (test_datagen_cpu.py, test_datagen_gpu.py): synthetic G-buffers whose alpha channel holds
every case the mask conversion distinguishes, the numpy restatement of the reference's ``convertToNumpy``, and clips with a coverage
pattern that makes the crop sampling reject some candidates."""
import numpy as np
import torch

import device_dataset_common as C

# what the renderer library starts with (csrc/gpu_renderer_direct.cpp: Args): a test that generated clips puts it back
RENDERER_DEFAULTS = (("semantics", "cpu"), ("cameraFoV", "45"), ("cameraOrigin", "0,0,-1"), ("cameraLookAt", "0,0,0"), ("cameraUp", "0,1,0"),
                     ("unshaded", "0"), ("resolution", "512,512"), ("viewport", "0,0,512,512"), ("isovalue", "0"), ("diffuse", "0.7,0.7,0.7"),
                     ("specular", "1,1,1"), ("exponent", "32"), ("light", "0,0,0"), ("light", "camera"), ("aosamples", "32"),
                     ("aoradius", "0.01"))
ALPHAS = (-0.5, -0.0, 0.0, 0.25, 1.0, 1.5, float("nan"), float("inf"), float("-inf"))


def synthetic_gbuffers(seed, h, w, r, nan=True):
    """(low [h, w, 12], high [r h, r w, 12], flow [2, h, w]) fp32 tensors: signed values with exact zeros of both signs, and an alpha
    channel cycling through below 0, -0, +0, inside, 1, above 1, NaN and the infinities (``nan=False``: without the NaN)."""
    rng = np.random.default_rng(seed)
    alphas = np.array([a for a in ALPHAS if nan or a == a], np.float32)
    out = []
    for H, W in ((h, w), (r * h, r * w)):
        g = rng.standard_normal((H, W, 12)).astype(np.float32)
        g[rng.random(g.shape) < 0.05] = 0.0
        g[rng.random(g.shape) < 0.05] = -0.0
        g[..., 3] = alphas[rng.integers(0, len(alphas), (H, W))]
        out.append(torch.from_numpy(g))
    flow = rng.standard_normal((2, h, w)).astype(np.float32)
    flow[rng.random(flow.shape) < 0.1] = -0.0
    return out[0], out[1], torch.from_numpy(flow)


def convert_to_numpy(gbuf, high):
    """``convertToNumpy`` (DataGenerator/DataGeneratorVideo2.py:66-77) for one image: the RGBA file clipped to [0, 1], its alpha as the
    mask in [-1, 1]; the normal / depth file and (high only) the first channel of the effects file unclipped."""
    planes = gbuf.transpose(2, 0, 1)
    rgb = np.clip(planes[0:4], 0, 1)
    parts = (rgb[3:4], planes[4:8]) + ((planes[10:11],) if high else ())
    out = np.concatenate(parts, axis=0)
    out[0, :, :] = out[0, :, :] * 2 - 1
    return out


def same_bits_with_nans(a, b):
    """``same_bits`` where neither is a NaN, and NaNs in the same places."""
    a, b = a.cpu(), b.cpu()
    nan = torch.isnan(a)
    zero = torch.zeros((), dtype=a.dtype)
    return torch.equal(nan, torch.isnan(b)) and C.same_bits(torch.where(nan, zero, a), torch.where(nan, zero, b))


def masked_clips(seed=21, sizes=((20, 24), (12, 17)), frames=3, crop=8, upscale=4):
    """Random clips (``device_dataset_common.random_clip``) of two sizes whose coverage sum ``low[0] + low[1] + low[2]`` is positive on
    the left part of frame 0 and on the upper part of frame T - 1 only, so that crops towards the lower right are rejected."""
    rng = np.random.default_rng(seed)
    clips = []
    for H, W in sizes:
        high, low, flow = C.random_clip(rng, frames, 5, 6, H, W, upscale)
        low[:, 0:3] = -np.abs(low[:, 0:3])
        low[0, 0:3, :, :W // 2 + 2] = np.abs(low[0, 0:3, :, :W // 2 + 2])
        low[frames - 1, 0:3, :H // 2 + 2, :] = np.abs(low[frames - 1, 0:3, :H // 2 + 2, :])
        clips.append((high, low, flow))
    return clips
