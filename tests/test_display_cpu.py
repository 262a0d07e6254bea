"""The display stage's definition (``viewer.compose_display``, ``viewer.focus_region``) against the reference viewer's frame, on the CPU.

``tests/golden/display_reference.npz`` (``tests/golden/make_display_fixtures.py``) holds what the reference's ``mainGUI.py`` lines compute,
around the reference's own ``F.interpolate``, ``VideoTools.warp_upscale`` and ``ScreenSpaceShading``, for the cases of
``tests/display_common.py``: every channel view, masking on and off, focus on and off, post-smoothing 0 and 0.5, a three-frame sequence
that feeds its displayed images back, and the colour-network route.

Measured when the fixture was made (fp32 reference against its own fp64, the premise) and against this package (profiles/display_stage.md):
premise 6.3e-7 at worst; ``compose_display`` against the fp32 fixture 3.0e-7 at worst."""
import os

import numpy as np
import pytest
import torch

import display_common as C
from isosurfacesuperresolution_amd import utils, viewer

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "display_reference.npz")
PREMISE = 2e-5            # the reference's fp32 against its own fp64: what a 1e-4 comparison of two fp32 evaluations presupposes
TOLERANCE = 1e-4          # the project's tolerance against the reference


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).unsqueeze(0)


def compose_case(case, k, prev, compose=viewer.compose_display, device="cpu", **extra):
    """One frame of a case of ``display_common.CASES`` through ``compose`` (the definition, or the kernel in tests/test_display_gpu.py)."""
    name, colournet, channel, masking, focus, factor, frames = case
    rgb, raw = C.network_output(k)
    gbuffer = torch.from_numpy(C.gbuffer(C.LOW_H, C.LOW_W, k)).permute(1, 2, 0).contiguous().to(device)
    kw = {}
    if focus:
        kw = dict(focus=viewer.focus_region(C.HIGH_H, C.HIGH_W, *C.focus_of(k), device=device),
                  focus_gbuffer=torch.from_numpy(C.gbuffer(C.HIGH_H, C.HIGH_W, k, detail=0.05)).permute(1, 2, 0).contiguous().to(device))
    return compose(gbuffer, _t(rgb).to(device), None if colournet else _t(raw).to(device), _t(C.filled_flow(k)).to(device),
                   shading=C.shading_for(utils.ScreenSpaceShading, device), channel=channel, masking=masking, background0=C.BACKGROUND0,
                   prev_displayed=prev, post_smoothing=factor, **{**kw, **extra})


def test_fixture_lists_the_cases_and_the_reference_is_close_to_its_own_fp64(golden):
    assert list(golden["cases"]) == [c[0] for c in C.CASES]
    views = {c[2] for c in C.CASES}
    assert views == set(viewer.CHANNELS)
    for on in (False, True):
        assert any(c[3] == on for c in C.CASES) and any(c[4] == on for c in C.CASES) and any((c[5] != 0) == on for c in C.CASES)
    for case in C.CASES:
        diff = golden[case[0] + "_fp64_minus_fp32"]
        assert diff.shape == golden[case[0]].shape and np.isfinite(diff).all()
        print("%-28s reference fp32 vs fp64 %.2e" % (case[0], np.abs(diff).max()))
        assert np.abs(diff).max() <= PREMISE, case[0]


@pytest.mark.parametrize("case", C.CASES, ids=[c[0] for c in C.CASES])
def test_compose_display_matches_the_reference(golden, case):
    name, colournet, channel, masking, focus, factor, frames = case
    ref = torch.from_numpy(golden[name])
    assert ref.shape[0] == len(frames) and tuple(ref.shape[-2:]) == (C.HIGH_H, C.HIGH_W)
    prev = None if len(frames) > 1 else _t(C.previous_image())
    for i, k in enumerate(frames):
        out = compose_case(case, k, prev)
        assert out.dtype == torch.float32 and tuple(out.shape) == (1, 3, C.HIGH_H, C.HIGH_W)
        if channel in C.SINGLE_PLANE_VIEWS:                        # (the fixture holds the first of the three planes)
            if factor == 0:                                        # ... which are one value; the smoothing blends each with its own previous plane
                assert torch.equal(out[:, 0], out[:, 1]) and torch.equal(out[:, 0], out[:, 2])
            got = out[0, 0:1]
        else:
            got = out[0]
        dist = (got - ref[i]).abs().max().item()
        print("%-28s frame %d: compose_display vs reference fp32 %.2e" % (name, k, dist))
        assert dist <= TOLERANCE, (name, k, dist)
        if len(frames) > 1:
            prev = ref[i].unsqueeze(0)            # the reference's own displayed image: every frame is a single step from the fixture


def test_sequence_fed_with_its_own_images_stays_at_the_reference(golden):
    """The same three frames with ``compose_display``'s OWN displayed images fed back, as ``DisplayStage`` does."""
    case = next(c for c in C.CASES if c[0] == "color_sequence")
    ref = torch.from_numpy(golden["color_sequence"])
    prev = None
    for i, k in enumerate(case[6]):
        prev = compose_case(case, k, prev)
        assert (prev[0] - ref[i]).abs().max().item() <= TOLERANCE


WINDOWS = ("inside", "corner00", "corner01", "corner10", "corner11", "huge", "blur_over_window")


@pytest.mark.parametrize("name", WINDOWS)
def test_focus_region_matches_the_reference_mask_and_viewport(golden, name):
    cx, cy, window, blur = (int(v) for v in golden["window_%s_args" % name])
    viewport, mask = viewer.focus_region(C.HIGH_H, C.HIGH_W, (cx, cy), window, blur)
    assert tuple(viewport) == tuple(int(v) for v in golden["window_%s_viewport" % name])
    ref = torch.from_numpy(golden["window_%s_mask" % name])
    assert mask.dtype == torch.float32 and tuple(mask.shape) == (1, C.HIGH_H, C.HIGH_W)
    assert (mask - ref).abs().max().item() <= 1e-6                # fp32 sqrt, subtract, divide: the same operations in numpy and torch
    x0, y0, x1, y1 = viewport
    assert 0 <= x0 <= x1 <= C.HIGH_W and 0 <= y0 <= y1 <= C.HIGH_H
    outside = torch.ones_like(mask, dtype=torch.bool)
    outside[:, y0:y1, x0:x1] = False
    assert not (mask[outside] > 0).any()                         # the blend never reaches a pixel that was not rendered


def test_focus_region_clamps_the_viewport():
    H, W = C.HIGH_H, C.HIGH_W
    assert viewer.focus_region(H, W, (3, 2), 10, 4)[0] == (0, 0, 13, 12)
    assert viewer.focus_region(H, W, (W - 3, 1), 10, 4)[0] == (W - 13, 0, W, 11)
    assert viewer.focus_region(H, W, (2, H - 2), 10, 4)[0] == (0, H - 12, 12, H)
    assert viewer.focus_region(H, W, (W - 2, H - 3), 10, 4)[0] == (W - 12, H - 13, W, H)
    assert viewer.focus_region(H, W, (40, 24), 200, 50)[0] == (0, 0, W, H)


def test_focus_region_without_blur_is_a_hard_edge():
    """The documented deviation: the reference divides by zero at ``blur == 0`` (NaN on the circle)."""
    _, mask = viewer.focus_region(C.HIGH_H, C.HIGH_W, (30, 20), 5, 0)
    assert torch.isfinite(mask).all() and set(mask.unique().tolist()) == {0.0, 1.0}
    assert mask[0, 20, 30] == 1 and mask[0, 20, 34] == 1 and mask[0, 20, 35] == 0 and mask[0, 17, 34] == 0 and mask[0, 23, 33] == 1
    assert int(mask.sum()) == 69                                   # lattice points with x^2 + y^2 < 25


def test_focus_region_with_a_blur_wider_than_the_window_ramps_from_the_centre():
    _, mask = viewer.focus_region(C.HIGH_H, C.HIGH_W, (40, 24), 12, 30)
    assert mask[0, 24, 40] == 1 and mask[0, 24, 46] == 0.5 and mask[0, 24, 52] == 0 and mask[0, 12, 40] == 0


def test_focus_select_keeps_what_lies_outside_the_viewport_out_of_the_arithmetic():
    case = next(c for c in C.CASES if c[0] == "normal_focus")
    plain = compose_case(case, 1, None)
    (x0, y0, x1, y1), _ = viewer.focus_region(C.HIGH_H, C.HIGH_W, *C.focus_of(1))
    full = torch.from_numpy(C.gbuffer(C.HIGH_H, C.HIGH_W, 1, detail=0.05)).permute(1, 2, 0).contiguous()
    poisoned = torch.full_like(full, float("nan"))
    poisoned[y0:y1, x0:x1] = full[y0:y1, x0:x1]
    out = compose_case(case, 1, None, focus_gbuffer=poisoned)
    assert torch.isfinite(out).all() and torch.equal(out, plain)


def test_uint8_presentation_and_bad_arguments():
    case = next(c for c in C.CASES if c[0] == "color_plain")
    out, rgba = compose_case(case, 1, None, present_uint8=True)
    assert rgba.dtype == torch.uint8 and tuple(rgba.shape) == (C.HIGH_H, C.HIGH_W, 4) and (rgba[..., 3] == 255).all()
    expect = np.round(np.clip(out[0].numpy().astype(np.float64), 0, 1).astype(np.float32) * np.float32(255)).astype(np.uint8)
    assert np.array_equal(rgba[..., :3].numpy(), expect.transpose(1, 2, 0))
    with pytest.raises(ValueError):
        compose_case(("x", False, "colour", False, False, 0.0, (1,)), 1, None)
