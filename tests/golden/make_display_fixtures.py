"""Generates tests/golden/display_reference.npz: the second half of the reference viewer's frame (mainGUI.py), case by case.

The reference's Python modules (`models`, `utils`) are IMPORTED from a checkout of the reference (its SuperresolutionNetwork directory,
given on the command line), unmodified, in the manner of make_colour_fixtures.py (torch CPU, one thread, deterministic algorithms,
`F.grid_sample` forced to `align_corners=True`).  `mainGUI.py` itself is a Tk program and cannot be imported: `reference_display` below
restates its lines 541-570 (focus bounds and mask), 603-608 / 626-628 (the twelve-channel image), 630-636 (masking), 787-798 (focus
blend), 803-828 (channel views) and 835-849 (post-smoothing) around the reference's own `F.interpolate` calls, `VideoTools.warp_upscale`
and `ScreenSpaceShading`.  The hole-filled flow is an INPUT (the reference fills with cv.inpaint, which is absent; the package's fill is
its own definition).  The inputs are the closed-form smooth fields of tests/display_common.py and are not stored.

Every case is evaluated in fp32 -- stored -- and in fp64 from the same fp32 inputs (a sequence: from the same fp32 previous image, a
single step), stored as its DIFFERENCE from the fp32 result in float32 (`<case>_fp64_minus_fp32`: fp32 + difference is the fp64 value to
1e-14; two float64 copies of every image would triple the file).  The reference's `ScreenSpaceShading` accumulates into a float32 tensor
and cannot run in fp64: `shade64` restates its formula for that evaluation only.  `VideoTools._offset_cache` is keyed by size alone and is
cleared between the two precisions.

Run:  python tests/golden/make_display_fixtures.py <reference checkout>/SuperresolutionNetwork
"""
import functools
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "display_reference.npz")
PREMISE = 2e-5                                # the reference's fp32 against its own fp64, every case
sys.path.insert(0, os.path.dirname(HERE))
import display_common as C                    # noqa: E402


def foc_bounds_and_mask(res_x, res_y, foc_center, window, blur, dtype):
    """mainGUI.py:541-570 (resX * upscale_factor = res_x, ...); `dtype`: np.float32 as the reference, np.float64 for the fp64 evaluation."""
    foc_x, foc_y = foc_center
    viewport = (max(0, foc_x - window), max(0, foc_y - window), min(res_x, foc_x + window), min(res_y, foc_y + window))
    outer_radius = window
    inner_radius = max(0, window - blur)

    def mask_fun(x, y):
        r = np.sqrt(np.square(x - foc_y) + np.square(y - foc_x))
        return np.clip((r - outer_radius) / (inner_radius - outer_radius), 0, 1)
    xaxis = np.linspace(0, res_y - 1, res_y, dtype=dtype)
    yaxis = np.linspace(0, res_x - 1, res_x, dtype=dtype)
    mask = mask_fun(xaxis[:, None], yaxis[None, :])
    return viewport, mask[np.newaxis, :, :]


def shade64(x):
    """utils/shading.py:148-191 in the dtype of `x` (the float32 colour vectors of C.SHADING, inverse_ao False, eye = (0, 0, 1))."""
    S = C.SHADING
    vec = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).to(torch.float32).to(x.dtype).view(1, 3, 1, 1)
    light = np.asarray(S["light"], dtype=np.float64)
    light = vec(light / np.linalg.norm(light))
    mask, normal = x[:, 0:1], x[:, 1:4]
    ao = S["ao"] * torch.clamp(x[:, 5:6], 0, 1) + (1 - S["ao"]) * torch.ones_like(x[:, 5:6])
    color = vec(S["ambient"]) * vec(S["material"]) + torch.zeros_like(normal)
    ndl = torch.sum(light * normal, dim=1, keepdim=True)
    color = color + (vec(S["diffuse"]) * vec(S["material"])) * torch.abs(ndl)
    reflect = 2 * ndl * normal - light
    spec = ((S["exponent"] + 2) / (2 * np.pi)) * (torch.clamp(reflect[:, 2:3], 0, 1) ** S["exponent"])
    color = (color + spec * vec(S["specular"])) * ao
    bg = vec(S["background"])
    return torch.clamp(bg + torch.clamp(mask * 0.5 + 0.5, 0, 1) * (color - bg), 0, 1)


def reference_display(VideoTools, shading, original_image, rgb, raw, flow, foc_image, foc, channel, masking, previous, factor):
    """One updateImage() after the network.  original_image [1,12,h,w] (mask in [0,1]); rgb: `self.shading(imageRaw)` / the clamped
    colour prediction; raw: `imageRaw` or None (a colour network); foc: (viewport, mask) or None; previous: previous_rgb_images or None."""
    image = torch.cat((original_image[:, 0:3], original_image[:, 3:4] * 2 - 1, original_image[:, 4:]), dim=1)      # :714-717
    image = F.interpolate(image, scale_factor=4, mode='bilinear')                                                   # :603 / :626
    base_mask = image[:, 3:4, :, :].clone()
    image[:, 0:3, :, :] = rgb                                                                                       # :606 / :628
    if raw is not None:
        image[:, 3:8, :, :] = raw[:, 0:-1, :, :]                                                                    # :607
        image[:, 10, :, :] = raw[:, -1, :, :]                                                                       # :608
    if masking:                                                                                                     # :630-636
        background = np.array([1, 1, 1])
        mask = (base_mask * 0.5 + 0.5)
        image = background[0] + mask * (image - background[0])
    if foc is not None:                                                                                             # :787-798
        _, mask = foc
        foc_image = torch.cat((foc_image[:, 0:3], foc_image[:, 3:4] * 2 - 1, foc_image[:, 4:]), dim=1)
        foc_image_shaded_input = torch.cat((foc_image[:, 3:4], foc_image[:, 4:8], foc_image[:, 10:11]), dim=1)
        foc_image_shaded = torch.clamp(shading(foc_image_shaded_input), 0, 1)
        foc_image[:, 0:3, :, :] = foc_image_shaded
        image = mask * foc_image + (1 - mask) * image
    if channel == "mask":                                                                                           # :803-828
        imageRGB = torch.cat((image[:, 3:4], image[:, 3:4], image[:, 3:4]), dim=1)
    elif channel == "normal":
        imageRGB = image[:, 4:7, :, :] * 0.5 + 0.5
    elif channel == "depth":
        depthVal = image[:, 7:8, :, :]
        depthForBounds = original_image[:, 7:8, :, :]
        maxDepth = torch.max(depthForBounds)
        minDepth = torch.min(depthForBounds + torch.le(depthForBounds, 1e-5).type_as(depthForBounds))
        depthVal = (depthVal - minDepth) / (maxDepth - minDepth)
        imageRGB = torch.cat((depthVal, depthVal, depthVal), dim=1)
    elif channel == "ao":
        imageRGB = torch.cat((image[:, 10:11], image[:, 10:11], image[:, 10:11]), dim=1)
    elif channel == "flow":
        flow_inpaint = torch.cat((flow, torch.zeros_like(flow[:, 0:1])), dim=1)
        imageRGB = (flow_inpaint * 10 + 0.5)
        imageRGB = F.interpolate(imageRGB, scale_factor=4, mode='bilinear')
    else:
        imageRGB = image[:, 0:3, :, :]
    if previous is not None and factor != 0:                                                                        # :835-849
        previous_warped = VideoTools.warp_upscale(previous, flow, 4)
        imageRGB = factor * previous_warped + (1 - factor) * imageRGB
    return imageRGB


def main():
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    warnings.filterwarnings("ignore")
    F.grid_sample = functools.partial(F.grid_sample, align_corners=True)
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "models")):
        sys.exit("usage: make_display_fixtures.py <reference checkout>/SuperresolutionNetwork")
    sys.path.insert(0, sys.argv[1])
    import models                                # noqa: F401
    import utils
    from models import VideoTools
    shading = C.shading_for(utils.ScreenSpaceShading, "cpu")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).unsqueeze(0)

    out = {"cases": np.array([c[0] for c in C.CASES])}
    # focGetBoundsAndMask for the windows the focus_region test looks at: name -> (centre, window, blur)
    windows = {"inside": ((30, 20), 14, 6), "corner00": ((3, 2), 10, 4), "corner01": ((77, 1), 10, 4), "corner10": ((2, 46), 10, 4),
               "corner11": ((78, 45), 10, 4), "huge": ((40, 24), 200, 50), "blur_over_window": ((40, 24), 12, 30)}
    for name, (centre, window, blur) in windows.items():
        vp, m = foc_bounds_and_mask(C.HIGH_W, C.HIGH_H, centre, window, blur, np.float32)
        assert m.dtype == np.float32
        out["window_%s_args" % name] = np.array([centre[0], centre[1], window, blur])
        out["window_%s_viewport" % name] = np.array(vp)
        out["window_%s_mask" % name] = m
    worst = 0.0
    for name, colournet, channel, masking, focus, factor, frames in C.CASES:
        prev32 = None if len(frames) > 1 else t(C.previous_image(), torch.float32)
        images, diffs = [], []
        for k in frames:
            rgb, raw = C.network_output(k)
            results = []
            for dt, npdt in ((torch.float32, np.float32), (torch.float64, np.float64)):
                VideoTools._offset_cache.clear()
                foc = None
                if focus:
                    vp, m = foc_bounds_and_mask(C.HIGH_W, C.HIGH_H, *C.focus_of(k), npdt)
                    foc = (vp, torch.from_numpy(m))
                with torch.no_grad():
                    results.append(reference_display(
                        VideoTools, shading if dt == torch.float32 else shade64, t(C.gbuffer(C.LOW_H, C.LOW_W, k), dt), t(rgb, dt),
                        None if colournet else t(raw, dt), t(C.filled_flow(k), dt), t(C.gbuffer(C.HIGH_H, C.HIGH_W, k, detail=0.05), dt),
                        foc, channel, masking, None if prev32 is None else prev32.to(dt), factor))
            r32, r64 = results
            assert r32.dtype == torch.float32 and r64.dtype == torch.float64
            worst = max(worst, (r32.double() - r64).abs().max().item())
            keep = slice(0, 1) if channel in C.SINGLE_PLANE_VIEWS else slice(0, 3)
            images.append(r32[0, keep].numpy())
            diffs.append((r64 - r32.double())[0, keep].numpy().astype(np.float32))
            if len(frames) > 1:
                prev32 = r32
        out[name] = np.stack(images)
        out[name + "_fp64_minus_fp32"] = np.stack(diffs)
        print("%-28s fp32 vs fp64: %.2e   range [%.3f, %.3f]" % (name, max(np.abs(d).max() for d in diffs), np.min(images), np.max(images)))
    assert worst <= PREMISE, "the reference itself is %g from fp64" % worst
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; worst fp32-fp64 distance %.2e" % worst)


if __name__ == "__main__":
    main()
