"""Generates tests/golden/render_modes_reference.npz: the reference viewer's frame in its four non-network render modes (mainGUI.py),
case by case.

As make_display_fixtures.py (which is imported for what it already restates): the reference's `models` and `utils` are IMPORTED from a
checkout of the reference given on the command line, unmodified (torch CPU, one thread, deterministic algorithms).  `mainGUI.py` is a Tk
program and cannot be imported: `reference_low_image` restates its lines 712-720 (the twelve-channel image of the rendered G-buffer, shaded
at the G-buffer's resolution) and `reference_upscale` its lines 732-752 (nearest / bilinear / bicubic `F.interpolate` of ALL twelve
channels; ground truth: the image as it is) around the reference's own `ScreenSpaceShading` and `F.interpolate`.  The rest of the frame
(focus blend :787-798, channel views :803-828, post-smoothing :835-849) is make_display_fixtures.reference_display, reused: handed the
image's channels 0:3 as `rgb` and 3:8, 10 as `raw` with masking off, it overwrites exactly the channels the views read with this
image's.  It resizes `original_image` by 4 first, which a ground-truth frame's full-resolution G-buffer cannot go through:
`ground_truth_view` restates :803-816, :828 for those cases (no focus window, no smoothing :835-838, bounds from the full-resolution
`original_image` :809-811).

Every case in fp32 -- stored -- and in fp64 from the same fp32 inputs, stored as its difference from the fp32 result (see
make_display_fixtures.py; `shade64` is its restatement of the shading for the fp64 evaluation).  The inputs are the closed-form fields
of tests/display_common.py (cases: tests/render_modes_common.py) and are not stored.

Run:  python tests/golden/make_render_mode_fixtures.py <reference checkout>/SuperresolutionNetwork
"""
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "render_modes_reference.npz")
sys.path.insert(0, HERE)
import make_display_fixtures as D            # noqa: E402  (puts tests/ on the path)
import display_common as C                    # noqa: E402
import render_modes_common as R               # noqa: E402

PREMISE = D.PREMISE


def reference_low_image(shading, image):
    """mainGUI.py:712-720; image [1,12,rows,cols], mask in [0,1]."""
    image = torch.cat((image[:, 0:3, :, :], image[:, 3:4, :, :] * 2 - 1, image[:, 4:, :, :]), dim=1)
    image_shaded_input = torch.cat((image[:, 3:4, :, :], image[:, 4:8, :, :], image[:, 10:11, :, :]), dim=1)
    image_shaded = torch.clamp(shading(image_shaded_input), 0, 1)
    image[:, 0:3, :, :] = image_shaded
    return image


def reference_upscale(image, mode):
    """mainGUI.py:732-752."""
    if mode == "nearest":
        return F.interpolate(image, scale_factor=4, mode='nearest')
    if mode == "bilinear":
        return F.interpolate(image, scale_factor=4, mode='bilinear')
    if mode == "bicubic":
        return F.interpolate(image, scale_factor=4, mode='bicubic')
    assert mode == "ground_truth"
    return image


def ground_truth_view(image, original_image, channel):
    """mainGUI.py:803-816, 828 on a ground-truth frame."""
    if channel == "mask":
        return torch.cat((image[:, 3:4], image[:, 3:4], image[:, 3:4]), dim=1)
    if channel == "normal":
        return image[:, 4:7, :, :] * 0.5 + 0.5
    if channel == "depth":
        depthVal = image[:, 7:8, :, :]
        depthForBounds = original_image[:, 7:8, :, :]
        maxDepth = torch.max(depthForBounds)
        minDepth = torch.min(depthForBounds + torch.le(depthForBounds, 1e-5).type_as(depthForBounds))
        depthVal = (depthVal - minDepth) / (maxDepth - minDepth)
        return torch.cat((depthVal, depthVal, depthVal), dim=1)
    if channel == "ao":
        return torch.cat((image[:, 10:11], image[:, 10:11], image[:, 10:11]), dim=1)
    assert channel == "color"
    return image[:, 0:3, :, :]


def main():
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    warnings.filterwarnings("ignore")
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "models")):
        sys.exit("usage: make_render_mode_fixtures.py <reference checkout>/SuperresolutionNetwork")
    import functools
    F.grid_sample = functools.partial(F.grid_sample, align_corners=True)
    sys.path.insert(0, sys.argv[1])
    import models                                # noqa: F401
    import utils
    from models import VideoTools
    shading = C.shading_for(utils.ScreenSpaceShading, "cpu")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).unsqueeze(0)

    out = {"cases": np.array([c[0] for c in R.CASES])}
    worst = 0.0
    for name, mode, channel, focus, factor, frames in R.CASES:
        prev32 = None if len(frames) > 1 else t(C.previous_image(), torch.float32)
        images, diffs = [], []
        for k in frames:
            results = []
            for dt, npdt in ((torch.float32, np.float32), (torch.float64, np.float64)):
                VideoTools._offset_cache.clear()
                shade = shading if dt == torch.float32 else D.shade64
                original_image = t(R.frame_gbuffer(mode, k), dt)
                with torch.no_grad():
                    image = reference_upscale(reference_low_image(shade, original_image), mode)
                    if mode == "ground_truth":
                        results.append(ground_truth_view(image, original_image, channel))
                        continue
                    foc = None
                    if focus:
                        vp, m = D.foc_bounds_and_mask(C.HIGH_W, C.HIGH_H, *C.focus_of(k), npdt)
                        foc = (vp, torch.from_numpy(m))
                    results.append(D.reference_display(
                        VideoTools, shade, original_image, image[:, 0:3], torch.cat((image[:, 3:8], image[:, 10:11]), dim=1),
                        t(C.filled_flow(k), dt), t(C.gbuffer(C.HIGH_H, C.HIGH_W, k, detail=0.05), dt), foc, channel, False,
                        None if prev32 is None else prev32.to(dt), factor))
            r32, r64 = results
            assert r32.dtype == torch.float32 and r64.dtype == torch.float64 and tuple(r32.shape) == (1, 3, C.HIGH_H, C.HIGH_W)
            worst = max(worst, (r32.double() - r64).abs().max().item())
            keep = slice(0, 1) if channel in R.SINGLE_PLANE_VIEWS else slice(0, 3)
            images.append(r32[0, keep].numpy())
            diffs.append((r64 - r32.double())[0, keep].numpy().astype(np.float32))
            if len(frames) > 1:
                prev32 = r32
        out[name] = np.stack(images)
        out[name + "_fp64_minus_fp32"] = np.stack(diffs)
        print("%-24s fp32 vs fp64: %.2e   range [%.3f, %.3f]" % (name, max(np.abs(d).max() for d in diffs), np.min(images), np.max(images)))
    assert worst <= PREMISE, "the reference itself is %g from fp64" % worst
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; worst fp32-fp64 distance %.2e" % worst)


if __name__ == "__main__":
    main()
