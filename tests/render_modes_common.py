"""Shared by tests/golden/make_render_mode_fixtures.py and the render-mode tests: the list of cases of the viewer's non-network render
modes (nearest, bilinear, bicubic, ground truth).  The inputs are the closed-form fields of tests/display_common.py at 12 x 20 -> 48 x 80
and are not stored: the frame's G-buffer is ``gbuffer(LOW_H, LOW_W, k)``, in ground truth ``gbuffer(HIGH_H, HIGH_W, k, detail=0.05)``,
which is also the focus window's full-resolution render.
"""
import display_common as C

# name, render mode, channel view, focus, post-smoothing factor, frames.  One-frame cases with smoothing blend with
# ``display_common.previous_image()``; the sequence starts without a previous image and feeds its own displayed images back.
CASES = (
    ("nearest_color", "nearest", "color", False, 0.0, (1,)),
    ("bilinear_color", "bilinear", "color", False, 0.0, (1,)),
    ("bicubic_color", "bicubic", "color", False, 0.0, (1,)),
    ("truth_color", "ground_truth", "color", False, 0.0, (1,)),
    ("bicubic_mask", "bicubic", "mask", False, 0.0, (1,)),
    ("bicubic_normal", "bicubic", "normal", False, 0.0, (1,)),
    ("bicubic_depth", "bicubic", "depth", False, 0.0, (1,)),
    ("bicubic_ao", "bicubic", "ao", False, 0.0, (1,)),
    ("bilinear_focus_smooth", "bilinear", "color", True, 0.5, (1,)),
    ("nearest_sequence", "nearest", "ao", False, 0.5, (0, 1, 2)),
    ("truth_depth", "ground_truth", "depth", False, 0.0, (1,)),
)
UNSHADED_VIEWS = ("mask", "normal", "depth", "ao")       # no shading enters: a few ulps from the reference, not the shading's 1e-4
SINGLE_PLANE_VIEWS = C.SINGLE_PLANE_VIEWS


def frame_gbuffer(mode, k):
    """[12, rows, cols]: the G-buffer the renderer hands over for frame k in ``mode``."""
    if mode == "ground_truth":
        return C.gbuffer(C.HIGH_H, C.HIGH_W, k, detail=0.05)
    return C.gbuffer(C.LOW_H, C.LOW_W, k)
