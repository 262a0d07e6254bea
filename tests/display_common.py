"""Shared by tests/golden/make_display_fixtures.py and the display-stage tests: the synthetic frame inputs and the list of cases.

The inputs are not stored in the fixture: they are closed-form, SMOOTH fields evaluated in float64 with +, -, *, / and sqrt only (IEEE
operations: the same values on every machine) and rounded once to float32.  Smooth on purpose -- a soft mask, low-frequency colours, a
small smooth flow: the reference's normalised-grid warp turns a 6e-8 rounding into 1e-4 across a hard edge, and the
fixture is to pin the composition, not that conditioning.
"""
import numpy as np

LOW_H, LOW_W = 12, 20
HIGH_H, HIGH_W = 4 * LOW_H, 4 * LOW_W
FRAMES = 3

# the shading set-up of pipeline.default_shading (white background: ``background[0]`` of the masking is 1)
SHADING = dict(fov=30.0, ambient=(0.1, 0.1, 0.1), diffuse=(0.8, 0.8, 0.8), specular=(0.02, 0.02, 0.02), exponent=16,
               light=(0.1, 0.1, 1.0), material=(1.0, 1.0, 1.0), ao=1.0, background=(1.0, 1.0, 1.0))
BACKGROUND0 = 1.0

# name, colour-network route, channel view, masking, focus, post-smoothing factor, frames.  One-frame cases with smoothing blend with
# ``previous_image()``; the sequence starts without a previous image and feeds its own displayed images back.
CASES = (
    ("color_plain", False, "color", False, False, 0.0, (1,)),
    ("mask_masked", False, "mask", True, False, 0.0, (1,)),
    ("normal_focus", False, "normal", False, True, 0.0, (1,)),
    ("depth_masked_focus_smooth", False, "depth", True, True, 0.5, (1,)),
    ("ao_focus_smooth", False, "ao", False, True, 0.5, (1,)),
    ("flow_smooth", False, "flow", False, False, 0.5, (1,)),
    ("color_sequence", False, "color", True, True, 0.5, (0, 1, 2)),
    ("colournet_masked", True, "color", True, False, 0.0, (1,)),
)
SINGLE_PLANE_VIEWS = ("mask", "depth", "ao")       # three equal planes: the fixture stores one


def focus_of(k):
    """(centre_xy, window, blur) of frame k: a window that moves with the sequence, partly blurred."""
    return (30 + 4 * k, 20 + 2 * k), 14, 6


def shading_for(cls, device="cpu"):
    """``SHADING`` on a ScreenSpaceShading class (the package's or the reference's: the same builder interface)."""
    s = cls(device)
    s.fov(SHADING["fov"])
    s.ambient_light_color(np.array(SHADING["ambient"]))
    s.diffuse_light_color(np.array(SHADING["diffuse"]))
    s.specular_light_color(np.array(SHADING["specular"]))
    s.specular_exponent(SHADING["exponent"])
    s.light_direction(np.array(SHADING["light"]))
    s.material_color(np.array(SHADING["material"]))
    s.ambient_occlusion(SHADING["ao"])
    s.background(np.array(SHADING["background"]))
    s.inverse_ao = False
    return s


def _fields(rows, cols, k):
    v = ((np.arange(rows, dtype=np.float64) + 0.5) / rows).reshape(rows, 1) * np.ones((1, cols))
    u = ((np.arange(cols, dtype=np.float64) + 0.5) / cols).reshape(1, cols) * np.ones((rows, 1))
    cx, cy = 0.45 + 0.03 * k, 0.5 + 0.02 * k
    px, py = (u - cx) / 0.4, (v - cy) / 0.45
    d2 = px * px + py * py
    s = np.clip(1.2 - d2, 0.0, 1.0)
    mask = s * s * (3.0 - 2.0 * s)                               # soft silhouette in [0, 1]
    nz = np.sqrt(np.clip(1.0 - 0.8 * d2, 0.05, 1.0))
    return u, v, d2, mask, 0.8 * px, 0.8 * py, nz


def gbuffer(rows, cols, k, detail=0.0):
    """A renderer G-buffer [12, rows, cols] of frame k: r g b mask nx ny nz depth fx fy ao shadow (mask in [0, 1]).  ``detail``: a
    low-frequency term that tells the full-resolution render of the focus window from the upscaled frame."""
    u, v, d2, mask, nx, ny, nz = _fields(rows, cols, k)
    e = detail * u * v
    rgb = np.stack([0.3 + 0.5 * u + e, 0.4 + 0.3 * v - e, 0.5 + 0.2 * u * v]) * mask
    n = np.stack([nx, ny, nz]) * mask
    depth = (0.35 + 0.2 * d2 + e) * mask
    flow = np.stack([0.012 + 0.004 * nx, -0.008 + 0.003 * ny]) * mask
    ao = (0.6 + 0.4 * nz - e) * mask
    return np.concatenate([rgb, mask[None], n, depth[None], flow, ao[None], mask[None]], axis=0).astype(np.float32)


def filled_flow(k):
    """[2, h, w]: the frame's flow, hole-filled -- an INPUT of the composition (the reference fills with cv.inpaint, the package with its
    own push-pull fill; neither is what this fixture pins): smooth and small everywhere."""
    u, v, *_ = _fields(LOW_H, LOW_W, k)
    return np.stack([0.012 + 0.004 * (u - 0.5) + 0.001 * k, -0.008 + 0.003 * (v - 0.5)]).astype(np.float32)


def network_output(k):
    """(rgb [3, H, W] in [0, 1], raw [6, H, W] clamped / normalised) as the pipeline hands them over: mask in [-1, 1], unit normal,
    depth and AO in [0, 1]."""
    u, v, d2, mask, nx, ny, nz = _fields(HIGH_H, HIGH_W, k)
    length = np.maximum(np.sqrt(nx * nx + ny * ny + nz * nz), 1e-7)
    raw = np.stack([2.0 * mask - 1.0, nx / length, ny / length, nz / length, np.clip((0.33 + 0.22 * d2) * mask, 0.0, 1.0),
                    np.clip((0.55 + 0.45 * nz) * mask, 0.0, 1.0)])
    rgb = np.clip(np.stack([0.25 + 0.6 * u * mask, 0.9 - 0.5 * v * mask, 0.35 + 0.5 * u * v]), 0.0, 1.0)
    return rgb.astype(np.float32), raw.astype(np.float32)


def previous_image():
    """[3, H, W]: a low-frequency previous displayed image for the one-frame cases."""
    u, v, *_ = _fields(HIGH_H, HIGH_W, 0)
    return np.stack([0.2 + 0.6 * u, 0.7 - 0.4 * v, 0.3 + 0.4 * u * v]).astype(np.float32)
