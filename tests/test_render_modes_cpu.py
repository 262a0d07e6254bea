"""The viewer's non-network render modes (``viewer.compose_baseline``, ``VideoTools.upscale_nearest`` / ``upscale_bicubic``) against the
reference viewer's frame, on the CPU.

``tests/golden/render_modes_reference.npz`` (``tests/golden/make_render_mode_fixtures.py``) holds what the reference's ``mainGUI.py``
lines 712-757 and the display half behind them compute, around the reference's own ``ScreenSpaceShading`` and ``F.interpolate``, for the
cases of ``tests/render_modes_common.py``.

Measured when the fixture was made: the reference's fp32 against its own fp64 (the premise) 4.8e-7 at worst; ``compose_baseline`` against
the fp32 fixture 2.4e-7 at worst in the colour views (bound 1e-4) and, in the unshaded views (bound 2e-6: a few ulps at the value range,
overshoot included -- the bicubic definition alone is up to 3.6e-7 from ``F.interpolate``), 2.4e-7 for bicubic and 4.8e-7 at worst, in
the third frame of the smoothed nearest sequence, where the warp's roundings add to the resize's (profiles/render_modes.md)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import display_common as C
import render_modes_common as R
from isosurfacesuperresolution_amd import utils, viewer
from isosurfacesuperresolution_amd.models.videotools import VideoTools

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_modes_reference.npz")
PREMISE = 2e-5            # the reference's fp32 against its own fp64
TOLERANCE = 1e-4          # the project's tolerance against the reference
UNSHADED = 2e-6           # the views no shading enters
SIZES = [(1, 9), (3, 2), (8, 8), (5, 64), (23, 37)]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).unsqueeze(0)


def compose_case(case, k, prev, compose=viewer.compose_baseline, device="cpu", **extra):
    """One frame of a case of ``render_modes_common.CASES`` through ``compose`` (the definition, or the launch in the GPU tests)."""
    name, mode, channel, focus, factor, frames = case
    gbuffer = torch.from_numpy(R.frame_gbuffer(mode, k)).permute(1, 2, 0).contiguous().to(device)
    kw = {}
    if focus:
        kw = dict(focus=viewer.focus_region(C.HIGH_H, C.HIGH_W, *C.focus_of(k), device=device),
                  focus_gbuffer=torch.from_numpy(C.gbuffer(C.HIGH_H, C.HIGH_W, k, detail=0.05)).permute(1, 2, 0).contiguous().to(device))
    kw.update(shading=C.shading_for(utils.ScreenSpaceShading, device), filled_flow=_t(C.filled_flow(k)).to(device), channel=channel,
              prev_displayed=prev, post_smoothing=factor)
    return compose(gbuffer, mode, **{**kw, **extra})


def test_fixture_lists_the_cases_and_the_reference_is_close_to_its_own_fp64(golden):
    assert list(golden["cases"]) == [c[0] for c in R.CASES]
    for mode in viewer.BASELINE_MODES:
        assert any(c[1] == mode and c[2] == "color" for c in R.CASES)
    assert {c[2] for c in R.CASES if c[1] == "bicubic"} >= {"mask", "normal", "depth", "ao"}
    assert any(c[3] and c[4] != 0 for c in R.CASES) and any(len(c[5]) == 3 and c[4] != 0 for c in R.CASES)
    assert any(c[1] == "ground_truth" and c[2] == "depth" for c in R.CASES)
    for case in R.CASES:
        diff = golden[case[0] + "_fp64_minus_fp32"]
        assert diff.shape == golden[case[0]].shape and np.isfinite(diff).all()
        print("%-24s reference fp32 vs fp64 %.2e" % (case[0], np.abs(diff).max()))
        assert np.abs(diff).max() <= PREMISE, case[0]


def _planes(out, channel):
    if channel in R.SINGLE_PLANE_VIEWS:                            # (the fixture holds the first of the three equal planes)
        assert torch.equal(out[:, 0], out[:, 1]) and torch.equal(out[:, 0], out[:, 2])
        return out[0, 0:1]
    return out[0]


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_compose_baseline_matches_the_reference(golden, case):
    name, mode, channel, focus, factor, frames = case
    ref = torch.from_numpy(golden[name])
    assert ref.shape[0] == len(frames) and tuple(ref.shape[-2:]) == (C.HIGH_H, C.HIGH_W)
    prev = None if len(frames) > 1 else _t(C.previous_image())
    bound = UNSHADED if channel in R.UNSHADED_VIEWS else TOLERANCE
    for i, k in enumerate(frames):
        out = compose_case(case, k, prev)
        assert out.dtype == torch.float32 and tuple(out.shape) == (1, 3, C.HIGH_H, C.HIGH_W)
        dist = (_planes(out, channel) - ref[i]).abs().max().item()
        print("%-24s frame %d: compose_baseline vs reference fp32 %.2e" % (name, k, dist))
        assert dist <= bound, (name, k, dist)
        if len(frames) > 1:
            prev = ref[i].expand(3, -1, -1).unsqueeze(0)            # the reference's own displayed image: every frame is a single step
    if mode == "bicubic" and channel in ("mask", "depth", "ao"):
        assert out.min().item() < (-1.0 if channel == "mask" else 0.0)   # the overshoot is kept: nothing clamps after the interpolation


def test_sequence_fed_with_its_own_images_stays_at_the_reference(golden):
    case = next(c for c in R.CASES if c[0] == "nearest_sequence")
    ref = torch.from_numpy(golden["nearest_sequence"])
    prev = None
    for i, k in enumerate(case[5]):
        prev = compose_case(case, k, prev)
        assert (prev[0, 0:1] - ref[i]).abs().max().item() <= UNSHADED


@pytest.mark.parametrize("h,w", SIZES + [(12, 20)])
def test_upscale_nearest_is_the_library_resize(h, w):
    x = torch.rand(2, 12, h, w, generator=torch.Generator().manual_seed(h * 100 + w)) * 2 - 1
    assert torch.equal(VideoTools.upscale_nearest(x, 4), F.interpolate(x, scale_factor=4, mode='nearest'))


@pytest.mark.parametrize("h,w", SIZES)
def test_upscale_bicubic_is_within_a_few_ulps_of_the_library_resize(h, w):
    x = torch.rand(2, 12, h, w, generator=torch.Generator().manual_seed(h * 100 + w)) * 2 - 1
    got = VideoTools.upscale_bicubic(x, 4)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 12, 4 * h, 4 * w)
    dist = (got - F.interpolate(x, scale_factor=4, mode='bicubic', align_corners=False)).abs().max().item()
    exact = (got.double() - F.interpolate(x.double(), scale_factor=4, mode='bicubic', align_corners=False)).abs().max().item()
    print("bicubic %dx%d: vs F.interpolate fp32 %.2e, vs fp64 %.2e" % (h, w, dist, exact))
    assert dist <= 2e-6 and exact <= 2e-6


def test_bicubic_weights_are_the_cubic_convolution_kernel_and_exact_in_fp32():
    A = -0.75
    c1 = lambda t: ((A + 2) * t - (A + 3)) * t * t + 1
    c2 = lambda t: ((A * t - 5 * A) * t + 8 * A) * t - 4 * A
    for phase, t in enumerate((0.625, 0.875, 0.125, 0.375)):
        row = VideoTools.BICUBIC_X4[phase]
        assert row == (c2(t + 1), c1(t), c1(1 - t), c2(2 - t))
        assert all(float(np.float32(v)) == v for v in row) and sum(row) == 1.0


def test_ground_truth_has_no_flow_view_no_window_and_no_smoothing():
    case = next(c for c in R.CASES if c[0] == "truth_color")
    with pytest.raises(ValueError):
        compose_case(("x", "ground_truth", "flow", False, 0.0, (1,)), 1, None)
    plain = compose_case(case, 1, None)
    region = viewer.focus_region(C.HIGH_H, C.HIGH_W, *C.focus_of(1))
    full = torch.full((C.HIGH_H, C.HIGH_W, 12), float("nan"))
    again = compose_case(case, 1, _t(C.previous_image()), focus=region, focus_gbuffer=full, post_smoothing=0.5)
    assert torch.equal(again, plain)


def test_unknown_mode_and_channel_raise_and_the_modes_have_no_masking():
    case = next(c for c in R.CASES if c[0] == "bilinear_color")
    with pytest.raises(ValueError):
        compose_case(("x", "network", "color", False, 0.0, (1,)), 1, None)
    with pytest.raises(ValueError):
        compose_case(("x", "bilinear", "colour", False, 0.0, (1,)), 1, None)
    with pytest.raises(TypeError):
        compose_case(case, 1, None, masking=True)                 # masking belongs to performSuperresolution: not an argument here


class _FakeRenderer:
    """Records the commands and fills the target with the case's G-buffer: what the stage needs of a renderer on the CPU."""

    def __init__(self):
        self.commands, self.renders, self.last = [], 0, None

    def send_command(self, cmd, value):
        self.commands.append((cmd, value))

    def set_last_camera(self, origin, lookat=(0.0, 0.0, 0.0)):
        self.last = tuple(origin)


def test_render_only_refuses_the_network_mode_and_masking_is_ignored_outside_it():
    shading = C.shading_for(utils.ScreenSpaceShading, "cpu")
    pipe = viewer.RenderOnly(_FakeRenderer(), shading, (C.LOW_W, C.LOW_H), device="cpu")
    assert pipe.upscale == 4 and (pipe.low_h, pipe.low_w) == (C.LOW_H, C.LOW_W) and tuple(pipe.gbuffer.shape) == (C.LOW_H, C.LOW_W, 12)
    with pytest.raises(ValueError):
        viewer.DisplayStage(pipe)                                  # the default mode is the network
    with pytest.raises(ValueError):
        viewer.DisplayStage(pipe, mode="cubic")
    stage = viewer.DisplayStage(pipe, mode="bicubic", masking=True, channel="mask")
    with pytest.raises(ValueError):
        stage.set_mode("network")
    assert stage.mode == "bicubic" and not stage.fused
    # the stage's composition of a stored frame (no render on the CPU): masking on or off, the same image -- the definition's
    g = torch.from_numpy(R.frame_gbuffer("bicubic", 1)).permute(1, 2, 0).contiguous()
    stage._frame_mode = "bicubic"
    state = (g, None, None, None, None, (0.0, 0.0, 1.0))
    masked = stage._compose(state, None, 0)
    stage.masking = False
    assert torch.equal(masked, stage._compose(state, None, 0))
    assert torch.equal(masked, viewer.compose_baseline(g, "bicubic", shading, channel="mask"))
