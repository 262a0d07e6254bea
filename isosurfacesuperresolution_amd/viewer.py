"""The display stage of the viewer's frame: focus-of-context, background masking, channel views, temporal post-smoothing.

``pipeline.SuperResolutionPipeline`` ends at the shaded RGB tensor.  This module is the rest of the reference viewer's frame loop
(``SuperresolutionNetwork/mainGUI.py:541-570, 603-608, 626-636, 762-853``), without its device -> host -> device trips (``cv.inpaint``
for the flow view and the smoothing, ``.cpu()`` at the end):

* ``focus_region``   -- ``focGetBoundsAndMask`` (``:541-570``): viewport and radial blending mask of the focus window;
* ``compose_display`` -- the frame after the network (``:603-608 / :626-628``, ``:630-636``, ``:787-798``, ``:803-828``, ``:835-849``),
  the DEFINITION: elementwise torch operations in fp32, one IEEE rounding each, order spelled out, as ``models/videotools.py`` and
  ``inference/flowfill.py`` are written.  ``csrc/sr_display.hip`` (``ops.display_frame``) computes the same bits wherever no shading
  enters and agrees to 1e-4 where the focus window is shaded (``tests/test_display_gpu.py``);
* ``compose_baseline`` -- the same frame in the viewer's four non-network render modes (``:84-91``, ``:681-693``, ``:712-757``): the
  rendered G-buffer shaded at its own resolution and interpolated x4 with all twelve channels (nearest, bilinear, bicubic), or rendered at
  full resolution (ground truth); the DEFINITION of ``ops.display_baseline_frame`` (``tests/test_render_modes_gpu.py``);
* ``DisplayStage``   -- the stage around a pipeline: one ``ops.display_frame`` launch per frame on device tensors; ``mode`` selects the
  network or one of the four other render modes (a render with the AO slider's samples, then ``ops.display_baseline_frame``);
* ``RenderOnly``     -- what the stage needs of a pipeline when there is no checkpoint: the four non-network modes without a model.

Deviations from the reference, all deliberate:

* the hole-filled flow is the package's own (``inference/flowfill.py``), the one the network's input was warped with, not ``cv.inpaint``;
* the x4 bilinear resize and the warp are the explicit forms of ``models/videotools.py`` (``upscale_bilinear``, ``warp_upscale``);
* ``blur == 0`` is a hard edge (the reference divides by zero there: NaN on the circle);
* where the focus mask is 0 the image is SELECTED, not multiplied by zero: pixels outside the rendered viewport never enter the arithmetic;
* the focus window is shaded with ``inverse_ao = False`` (its AO comes from the renderer), which is what the reference does on its
  ``only_foc_changed`` path; on the full path it leaves the model's flag set;
* the x4 nearest and bicubic resizes of the render modes are the explicit forms of ``models/videotools.py`` (``upscale_nearest``: equal to
  ``F.interpolate``; ``upscale_bicubic``: ATen's taps and weights in a fixed operation order, a few 1e-7 from ``F.interpolate``);
* ground-truth mode has no flow view (``ValueError``): the reference resizes the already full-resolution flow by 4 once more there, which
  is a bug and not a contract; and it has no focus window, which would show the same render.
"""
import numpy as np
import torch

from . import ops
from .models.videotools import VideoTools
from .volumes import fmt3

CHANNELS = ("color", "mask", "normal", "depth", "ao", "flow")
BASELINE_MODES = ("nearest", "bilinear", "bicubic", "ground_truth")
MODES = ("network",) + BASELINE_MODES          # mainGUI.py:84-91


def focus_region(H, W, centre_xy, window, blur, device="cpu"):
    """``mainGUI.py:541-570``: -> (viewport (minX, minY, maxX, maxY), mask [1, H, W] fp32 with 1 = full-resolution render).
    ``r = sqrt((Y - cy)^2 + (X - cx)^2)``, ``m = clip((r - outer) / (inner - outer), 0, 1)`` with ``outer = window`` and
    ``inner = max(0, window - blur)``, in fp32 like the reference's numpy.  ``blur == 0``: ``m = 1`` where ``r < outer``, else 0."""
    cx, cy = centre_xy
    # (the reference clamps the minima at 0 and the maxima at the image; a window wholly off the image is kept empty, not negative)
    viewport = (min(int(W), max(0, int(cx - window))), min(int(H), max(0, int(cy - window))),
                max(0, min(int(W), int(cx + window))), max(0, min(int(H), int(cy + window))))
    outer = float(window)
    inner = float(max(0, window - blur))
    ys = torch.arange(H, dtype=torch.float32, device=device).view(H, 1)
    xs = torch.arange(W, dtype=torch.float32, device=device).view(1, W)
    dy, dx = ys - float(cy), xs - float(cx)
    r = torch.sqrt(dy * dy + dx * dx)
    if inner == outer:
        m = (r < outer).to(torch.float32)
    else:
        m = ((r - outer) / (inner - outer)).clamp(0, 1)
    return viewport, m.unsqueeze(0)


def depth_bounds(gbuffer):
    """(min, max) of the frame's depth as the depth view normalises with them (``mainGUI.py:809-811``): ``max(d)`` and
    ``min(d + (d <= 1e-5))`` over the G-buffer rendered for the frame -- the LOW-resolution one [h, w, 12], in ground-truth mode the
    full-resolution one; a two-float tensor on the G-buffer's device (no host read)."""
    d = gbuffer[..., 7]
    return torch.stack([(d + (d <= 1e-5).to(d.dtype)).min(), d.max()])


def _focus_image(focus_gbuffer, shading):
    """Full-resolution G-buffer [H, W, 12] -> the reference's twelve-channel ``foc_image`` [1, 12, H, W] (``mainGUI.py:787-795``); the
    same lines make the render modes' image of a G-buffer of either resolution (``:712-720``)."""
    f = focus_gbuffer.permute(2, 0, 1).unsqueeze(0)
    f = torch.cat([f[:, 0:3], f[:, 3:4] * 2.0 - 1.0, f[:, 4:]], dim=1)
    saved = shading.inverse_ao
    shading.inverse_ao = False
    try:
        shaded = torch.clamp(shading(torch.cat([f[:, 3:4], f[:, 4:8], f[:, 10:11]], dim=1)), 0, 1)
    finally:
        shading.inverse_ao = saved
    return torch.cat([shaded, f[:, 3:]], dim=1)


def to_uint8(image):
    """[1, 3, H, W] -> RGBA [H, W, 4] uint8: ``round(clamp(x, 0, 1) * 255)``, A = 255."""
    rgb = (image[0].clamp(0, 1) * 255.0).round().to(torch.uint8).permute(1, 2, 0)
    return torch.cat([rgb, torch.full_like(rgb[..., :1], 255)], dim=2).contiguous()


def compose_display(gbuffer, rgb, raw=None, filled_flow=None, shading=None, channel="color", masking=False, background0=1.0,
                    focus=None, focus_gbuffer=None, bounds=None, prev_displayed=None, post_smoothing=0.0, present_uint8=False):
    """The frame after the network, for both model families.

    gbuffer [h, w, 12]: the renderer's low-resolution G-buffer (mask in [0, 1]); rgb [1, 3, H, W]: the shaded network output, or a
    colour network's clamped prediction; raw [1, 6, H, W] (unshaded networks; None: colour networks); filled_flow [1, 2, h, w];
    focus: ``focus_region``'s (viewport, mask) with focus_gbuffer [H, W, 12] and ``shading``; bounds: ``depth_bounds(gbuffer)`` (computed
    if None); prev_displayed [1, 3, H, W].  -> displayed [1, 3, H, W] (, RGBA uint8 [H, W, 4] with ``present_uint8``).

    1. image: 12 channels, x4 bilinear of the low G-buffer with its mask mapped to +-1; 0:3 <- rgb, and with ``raw`` 3:8 <- raw[0:5],
       10 <- raw[5].  2. masking: bg0 + t (image - bg0), t = base_mask 0.5 + 0.5 (the upscaled mask).  3. focus: image = m foc +
       (1 - m) image where m > 0 inside the viewport.  4. channel view.  5. f32 warp_upscale(prev, flow, 4) + g32 image.  6. 8 bit."""
    if channel not in CHANNELS:
        raise ValueError("channel must be one of %s" % (CHANNELS,))
    dtype, device = torch.float32, gbuffer.device
    low = gbuffer.permute(2, 0, 1).unsqueeze(0)
    low = torch.cat([low[:, 0:3], low[:, 3:4] * 2.0 - 1.0, low[:, 4:]], dim=1)
    image = VideoTools.upscale_bilinear(low, 4)
    base_mask = image[:, 3:4]
    if raw is not None:
        image = torch.cat([rgb, raw[:, 0:5], image[:, 8:10], raw[:, 5:6], image[:, 11:12]], dim=1)
    else:
        image = torch.cat([rgb, image[:, 3:]], dim=1)
    if masking:
        bg0 = torch.full((), float(background0), dtype=dtype, device=device)
        t = base_mask * 0.5 + 0.5
        image = bg0 + t * (image - bg0)
    return _finish_display(image, gbuffer, filled_flow, shading, channel, focus, focus_gbuffer, bounds, prev_displayed, post_smoothing,
                           present_uint8)


def _finish_display(image, gbuffer, filled_flow, shading, channel, focus, focus_gbuffer, bounds, prev_displayed, post_smoothing, present_uint8):
    """Steps 3 to 6 of ``compose_display`` on the twelve-channel ``image`` [1, 12, H, W]; shared with ``compose_baseline``."""
    dtype, device = torch.float32, gbuffer.device
    if focus is not None:
        (x0, y0, x1, y1), m = focus
        H, W = image.shape[-2:]
        m = m.to(device).view(1, 1, H, W)
        inside = torch.zeros((1, 1, H, W), dtype=torch.bool, device=device)
        inside[:, :, y0:y1, x0:x1] = True
        foc = _focus_image(focus_gbuffer, shading)
        image = torch.where(inside & (m > 0), m * foc + (1.0 - m) * image, image)
    if channel == "mask":
        out = torch.cat([image[:, 3:4]] * 3, dim=1)
    elif channel == "normal":
        out = image[:, 4:7] * 0.5 + 0.5
    elif channel == "depth":
        if bounds is None:
            bounds = depth_bounds(gbuffer)
        d = (image[:, 7:8] - bounds[0]) / (bounds[1] - bounds[0])
        out = torch.cat([d, d, d], dim=1)
    elif channel == "ao":
        out = torch.cat([image[:, 10:11]] * 3, dim=1)
    elif channel == "flow":
        f3 = torch.cat([filled_flow, torch.zeros_like(filled_flow[:, 0:1])], dim=1)
        out = VideoTools.upscale_bilinear(f3 * 10.0 + 0.5, 4)
    else:
        out = image[:, 0:3]
    if prev_displayed is not None and post_smoothing != 0:
        f32 = torch.full((), float(np.float32(post_smoothing)), dtype=dtype, device=device)
        g32 = torch.full((), float(np.float32(1.0 - post_smoothing)), dtype=dtype, device=device)
        out = f32 * VideoTools.warp_upscale(prev_displayed, filled_flow, 4) + g32 * out
    out = out.contiguous()
    return (out, to_uint8(out)) if present_uint8 else out


def compose_baseline(gbuffer, mode, shading, filled_flow=None, channel="color", focus=None, focus_gbuffer=None, bounds=None,
                     prev_displayed=None, post_smoothing=0.0, present_uint8=False):
    """The frame of the viewer's non-network render modes (``mainGUI.py:712-757``, then as ``compose_display`` from step 3 on).

    gbuffer: the G-buffer rendered for this frame (with the AO slider's samples; mask in [0, 1]) -- [h, w, 12], in ``ground_truth``
    [4h, 4w, 12]; mode: one of ``BASELINE_MODES``; the other arguments as ``compose_display``; bounds: ``depth_bounds(gbuffer)`` of
    THIS G-buffer.  -> displayed [1, 3, 4h, 4w] (, RGBA uint8).

    1. L: twelve channels at the G-buffer's resolution, mask mapped to +-1, 0:3 = clamp(shading(mask, normal, depth, ao), 0, 1) with
       ``inverse_ao = False``.  2. image = ``upscale_nearest`` / ``upscale_bilinear`` / ``upscale_bicubic`` (L, 4), ALL twelve channels
       (the colour is interpolated, not shaded again; nothing is clamped: the bicubic overshoot stays until the 8-bit output), or L itself
       in ``ground_truth``.  No background masking.  3. - 6. as ``compose_display``; ``ground_truth`` skips the focus window (it would
       show the same render) and the post-smoothing (``:835-838``), and has no flow view (``ValueError``; see the module docstring)."""
    if mode not in BASELINE_MODES:
        raise ValueError("mode must be one of %s" % (BASELINE_MODES,))
    if channel not in CHANNELS:
        raise ValueError("channel must be one of %s" % (CHANNELS,))
    image = _focus_image(gbuffer, shading)
    if mode == "ground_truth":
        if channel == "flow":
            raise ValueError("compose_baseline: no flow view in ground-truth mode")
        focus = focus_gbuffer = prev_displayed = None
    elif mode == "nearest":
        image = VideoTools.upscale_nearest(image, 4)
    elif mode == "bilinear":
        image = VideoTools.upscale_bilinear(image, 4)
    else:
        image = VideoTools.upscale_bicubic(image, 4)
    return _finish_display(image, gbuffer, filled_flow, shading, channel, focus, focus_gbuffer, bounds, prev_displayed, post_smoothing,
                           present_uint8)


class DisplayStage:
    """The display half of the viewer's frame around a ``SuperResolutionPipeline``.

    ``frame(origin, next_origin)`` runs ``pipeline.frame``, renders the focus window (if any) at full resolution with ray-cast AO, and
    composes the displayed image in ONE launch (``ops.display_frame``); the displayed tensor is the next frame's "previous" of the
    post-smoothing.  ``refocus(focus)`` is the reference's ``only_foc_changed`` path: the window is rendered again and the stored frame
    recomposed -- no network, and the smoothing state does not advance.  CPU pipelines and ``fused=False`` run ``compose_display``.

    ``focus``: None or ``(centre_xy, window, blur)`` in high-resolution pixels.  Returned tensors are valid until the frame after next.

    ``mode`` (``set_mode``; one of ``MODES``, default "network": the above): in "nearest", "bilinear", "bicubic" and "ground_truth" no
    network runs (``mainGUI.py:681-693, 732-752``).  The frame is rendered on the current stream with ``ao_samples`` / ``ao_radius`` -- at
    low resolution into the pipeline's G-buffer slot, in ground truth at full resolution into a buffer of the stage's -- and composed by
    ``ops.display_baseline_frame`` (``compose_baseline`` on the CPU and with ``fused=False``).  A render the pipeline had started ahead
    is dropped (it was made without AO) and ``next_origin`` is ignored; the network's recurrence is cleared, so the next network frame
    is the first of a sequence; ``masking`` does not apply; the displayed image advances in every mode and is smoothed in all but
    ground truth.  A frame's flow is measured against the camera of the frame displayed before it, whichever mode showed that one."""

    def __init__(self, pipeline, channel="color", masking=False, post_smoothing=0.0, focus=None, focus_ao_samples=0, focus_ao_radius=0.01,
                 present_uint8=False, fused=True, mode="network", ao_samples=0, ao_radius=0.01):
        if getattr(pipeline, "graph", False):
            raise NotImplementedError("DisplayStage: a pipeline that replays its frame as a HIP graph (graph=True) is not supported")
        if channel not in CHANNELS:
            raise ValueError("channel must be one of %s" % (CHANNELS,))
        self.pipeline = pipeline
        self.channel = channel
        self.masking = bool(masking)
        self.post_smoothing = float(post_smoothing)
        self.focus_ao_samples = int(focus_ao_samples)
        self.focus_ao_radius = float(focus_ao_radius)
        self.ao_samples = int(ao_samples)
        self.ao_radius = float(ao_radius)
        self.present_uint8 = bool(present_uint8)
        self.device = torch.device(pipeline.device)
        self.fused = bool(fused) and self.device.type == "cuda"
        self.H, self.W = pipeline.upscale * pipeline.low_h, pipeline.upscale * pipeline.low_w
        if pipeline.upscale != 4:
            raise NotImplementedError("DisplayStage: x4 pipelines only")
        self.previous = None              # the last DISPLAYED image (post-smoothing state)
        self._frame_state = None          # (gbuffer, rgb, raw, flow, bounds, previous displayed at that time, origin) of the last frame
        # displayed images: two alternate (the warp reads the previous one while this one is written), the third is refocus()'s
        self._out = [None, None, None]
        self._out8 = [None, None, None]
        self._turn = 0
        self._prev_at_frame = None        # the displayed image BEFORE the stored frame: what refocus() smooths against
        self._focus_gbuffer = None
        self._truth_gbuffer = None        # ground-truth mode's full-resolution render
        self._low_planes = None           # workspace of ops.display_baseline_frame's pre-pass
        self._frame_mode = None           # the mode that showed the stored frame
        self.set_mode(mode)
        self.set_focus(focus)

    def set_mode(self, mode):
        """The render mode of the frames to come (``mainGUI.py:84-91``); a stored frame stays what it was for ``refocus``."""
        if mode not in MODES:
            raise ValueError("mode must be one of %s" % (MODES,))
        if mode == "network" and getattr(self.pipeline, "model", None) is None:
            raise ValueError("DisplayStage: the network mode needs a pipeline with a model")
        self.mode = mode

    def set_focus(self, focus):
        self.focus = focus
        self._region = None
        if focus is not None:
            centre, window, blur = focus
            self._region = focus_region(self.H, self.W, centre, window, blur, device=self.device)

    def reset(self, flush=True):
        """New temporal sequence: forwards to the pipeline and drops the previous displayed image."""
        self.pipeline.reset(flush=flush)
        self.previous = None
        self._frame_state = None
        self._frame_mode = None
        self._prev_at_frame = None

    # ---- focus render ----------------------------------------------------------------------------------------------------------
    def _render_focus(self, origin):
        """The full-resolution G-buffer of ``origin`` inside the focus viewport, on the current stream (``mainGUI.py:766-785``), into a
        reused [H, W, 12] buffer; the renderer is left as the pipeline set it up, its flow reference ("last camera") included."""
        pipe, r = self.pipeline, self.pipeline.renderer
        if self._focus_gbuffer is None:
            self._focus_gbuffer = torch.zeros((self.H, self.W, 12), dtype=torch.float32, device=self.device)
        cur = torch.cuda.current_stream()
        if pipe._prefetched is not None:
            # the next frame's render is in flight on the side stream: the renderer's launches share its tile queue -- one at a time
            cur.wait_event(pipe._ready[pipe._prefetched[1]])
        viewport = self._region[0]
        r.send_command("cameraOrigin", fmt3(origin))
        r.send_command("resolution", "%d,%d" % (self.W, self.H))
        r.send_command("viewport", "%d,%d,%d,%d" % viewport)
        r.send_command("aoradius", "%5.3f" % self.focus_ao_radius)
        r.send_command("aosamples", "%d" % self.focus_ao_samples)
        try:
            r.render_async(self._focus_gbuffer, cur)
        finally:
            r.send_command("resolution", "%d,%d" % (pipe.low_w, pipe.low_h))
            r.send_command("viewport", "%d,%d,%d,%d" % (0, 0, pipe.low_w, pipe.low_h))
            r.send_command("aoradius", "%5.3f" % 0.01)
            r.send_command("aosamples", "0")
            # a render moves the flow reference: with frame t+1 already rendered ahead, frame t+2's flow must be measured against t+1
            last = pipe._prefetched[0] if pipe._prefetched is not None else pipe._displayed
            if last is not None:
                r.set_last_camera(tuple(float(v) for v in fmt3(last).split(",")), pipe._lookat)
        return self._focus_gbuffer

    # ---- composition -----------------------------------------------------------------------------------------------------------
    def _compose(self, state, prev, slot):
        gbuffer, rgb, raw, flow, bounds, origin = state
        if self._frame_mode != "network":
            return self._compose_baseline(state, prev, slot)
        colour = self.pipeline.colour
        focus_g = None
        if self._region is not None:
            focus_g = self._render_focus(origin)
        smoothing = self.post_smoothing if prev is not None else 0.0
        if not self.fused:
            return compose_display(gbuffer, rgb, None if colour else raw, flow, shading=self.pipeline.shading, channel=self.channel,
                                   masking=self.masking, background0=self._background0(), focus=self._region, focus_gbuffer=focus_g,
                                   bounds=bounds, prev_displayed=prev if smoothing != 0 else None, post_smoothing=smoothing,
                                   present_uint8=self.present_uint8)
        if self._out[slot] is None:
            self._out[slot] = torch.empty((1, 3, self.H, self.W), dtype=torch.float32, device=self.device)
        if self.present_uint8 and self._out8[slot] is None:
            self._out8[slot] = torch.empty((self.H, self.W, 4), dtype=torch.uint8, device=self.device)
        out = ops.display_frame(gbuffer, rgb, None if colour else raw, flow, shading=self.pipeline.shading, channel=self.channel,
                                masking=self.masking, background0=self._background0(), focus=self._region, focus_gbuffer=focus_g,
                                bounds=bounds, prev_displayed=prev if smoothing != 0 else None, post_smoothing=smoothing,
                                out=self._out[slot], out8=self._out8[slot] if self.present_uint8 else None)
        return (out, self._out8[slot]) if self.present_uint8 else out

    def _compose_baseline(self, state, prev, slot):
        gbuffer, _, _, flow, bounds, origin = state
        mode = self._frame_mode
        truth = mode == "ground_truth"
        focus_g = None
        region = None if truth else self._region             # (ground truth: the window would show the same render)
        if region is not None:
            focus_g = self._render_focus(origin)
        smoothing = self.post_smoothing if prev is not None and not truth else 0.0
        if smoothing != 0 and flow is None:                  # (refocus after post_smoothing was switched on: the stored frame has no flow)
            smoothing = 0.0
        kw = dict(shading=self.pipeline.shading, filled_flow=flow, channel=self.channel, focus=region, focus_gbuffer=focus_g, bounds=bounds,
                  prev_displayed=prev if smoothing != 0 else None, post_smoothing=smoothing)
        if not self.fused:
            return compose_baseline(gbuffer, mode, present_uint8=self.present_uint8, **kw)
        if self._out[slot] is None:
            self._out[slot] = torch.empty((1, 3, self.H, self.W), dtype=torch.float32, device=self.device)
        if self.present_uint8 and self._out8[slot] is None:
            self._out8[slot] = torch.empty((self.H, self.W, 4), dtype=torch.uint8, device=self.device)
        if self._low_planes is None and not truth:
            self._low_planes = torch.empty((12, self.H // 4, self.W // 4), dtype=torch.float32, device=self.device)
        out = ops.display_baseline_frame(gbuffer, mode, out=self._out[slot], out8=self._out8[slot] if self.present_uint8 else None,
                                         workspace=None if truth else self._low_planes, **kw)
        return (out, self._out8[slot]) if self.present_uint8 else out

    def _background0(self):
        return float(self.pipeline.shading.packed_parameters()[15])

    def _render_mode_frame(self, origin):
        """The G-buffer of a non-network frame, rendered on the current stream with the AO slider's parameters (``mainGUI.py:681-693``):
        low resolution into the pipeline's G-buffer slot, ground truth into a reused [H, W, 12] buffer.  The renderer's resolution,
        viewport and AO parameters are put back; its "last camera" is now this frame's, and this frame is the displayed one."""
        pipe, r = self.pipeline, self.pipeline.renderer
        truth = self.mode == "ground_truth"
        cur = torch.cuda.current_stream()
        if pipe._prefetched is not None:
            # a render made ahead for the network (without AO) is not shown: wait for it (the renderer's launches share its tile queue),
            # forget it, and put the flow reference back to the frame displayed last
            cur.wait_event(pipe._ready[pipe._prefetched[1]])
            pipe._drop_prefetched()
        if truth:
            if self._truth_gbuffer is None:
                self._truth_gbuffer = torch.zeros((self.H, self.W, 12), dtype=torch.float32, device=self.device)
            target, (rw, rh) = self._truth_gbuffer, (self.W, self.H)
        else:
            pipe._flow_ready[pipe._slot] = False
            pipe.gbuffer = pipe._gbuffers[pipe._slot]
            target, (rw, rh) = pipe.gbuffer, (pipe.low_w, pipe.low_h)
        r.send_command("cameraOrigin", fmt3(origin))
        r.send_command("resolution", "%d,%d" % (rw, rh))
        r.send_command("viewport", "%d,%d,%d,%d" % (0, 0, rw, rh))
        r.send_command("aoradius", "%5.3f" % self.ao_radius)
        r.send_command("aosamples", "%d" % self.ao_samples)
        try:
            r.render_async(target, cur)
        finally:
            r.send_command("resolution", "%d,%d" % (pipe.low_w, pipe.low_h))
            r.send_command("viewport", "%d,%d,%d,%d" % (0, 0, pipe.low_w, pipe.low_h))
            r.send_command("aoradius", "%5.3f" % 0.01)
            r.send_command("aosamples", "0")
        pipe._displayed = tuple(float(v) for v in fmt3(origin).split(","))       # what the renderer parsed: the next frame's flow reference
        return target

    def _baseline_frame(self, origin):
        pipe = self.pipeline
        truth = self.mode == "ground_truth"
        if truth and self.channel == "flow":
            raise ValueError("DisplayStage: no flow view in ground-truth mode")
        with torch.no_grad():
            gbuffer = self._render_mode_frame(origin)
            pipe.previous = None              # mainGUI.py:737-752: the network's recurrence starts over at its next frame (no flush)
            flow = None
            if self.channel == "flow" or (self.previous is not None and self.post_smoothing != 0 and not truth):
                if self.fused:
                    flow = ops.fill_flow_gbuffer(gbuffer)
                else:
                    from .inference.flowfill import fill_flow
                    low = gbuffer.permute(2, 0, 1).unsqueeze(0)
                    flow = fill_flow(low[:, 8:10], low[:, 3:4])
            bounds = depth_bounds(gbuffer) if self.channel == "depth" else None
            self._frame_state = (gbuffer, None, None, flow, bounds, tuple(origin))
            self._frame_mode = self.mode
            self._prev_at_frame = self.previous
            self._turn ^= 1
            result = self._compose(self._frame_state, self.previous, self._turn)
            self.previous = result[0] if self.present_uint8 else result
        return result

    def frame(self, origin, next_origin=None):
        if self.mode != "network":
            return self._baseline_frame(origin)
        pipe = self.pipeline
        with torch.no_grad():
            rgb, raw = pipe.frame(origin, next_origin)
            gbuffer = pipe.gbuffer
            need_flow = self.channel == "flow" or (self.previous is not None and self.post_smoothing != 0)
            flow = None
            if need_flow:
                if pipe.fused and pipe._flow_ready[pipe._slot]:
                    flow = pipe._flows[pipe._slot]
                elif self.fused:
                    flow = ops.fill_flow_gbuffer(gbuffer)
                else:
                    from .inference.flowfill import fill_flow
                    low = gbuffer.permute(2, 0, 1).unsqueeze(0)
                    flow = fill_flow(low[:, 8:10], low[:, 3:4])
            bounds = depth_bounds(gbuffer) if self.channel == "depth" else None
            self._frame_state = (gbuffer, rgb, raw, flow, bounds, tuple(origin))
            self._frame_mode = "network"
            self._prev_at_frame = self.previous
            self._turn ^= 1
            result = self._compose(self._frame_state, self.previous, self._turn)
            self.previous = result[0] if self.present_uint8 else result
        return result

    def refocus(self, focus):
        """``only_foc_changed`` (``mainGUI.py:758-760``): another focus window over the stored frame -- the window is rendered again, the
        frame recomposed against the image displayed BEFORE it; no network runs and no low-resolution render (a ground-truth frame is
        recomposed without a window).  The result lives in a buffer of its own, valid until
        the next ``refocus``; the smoothing state (``self.previous``, the image ``frame`` returned) does not advance.  To be called
        before the pipeline's next ``frame``."""
        if self._frame_state is None:
            raise RuntimeError("refocus: no frame to recompose")
        self.set_focus(focus)
        with torch.no_grad():
            return self._compose(self._frame_state, self._prev_at_frame, 2)


class RenderOnly:
    """What ``DisplayStage`` needs of a pipeline when there is no checkpoint (the reference's ``--model`` defaults to None and its GUI
    still renders): the renderer, the shading, the low resolution, one G-buffer slot, ``set_static`` and ``reset``.  A stage on it takes
    the four non-network modes; ``mode="network"`` raises ``ValueError``."""

    model = None
    colour = False
    graph = False
    upscale = 4

    def __init__(self, renderer, shading, low_res, device="cuda"):
        self.renderer = renderer
        self.shading = shading
        self.low_w, self.low_h = low_res
        self.device = device
        self.gbuffer = torch.empty((self.low_h, self.low_w, 12), dtype=torch.float32, device=device)
        self._gbuffers = [self.gbuffer]
        self._flow_ready = [False]
        self._slot = 0
        self._prefetched = None           # nothing is rendered ahead: no network beside which a render could hide
        self._displayed = None            # origin of the frame displayed last: the flow reference
        self.previous = None
        self.set_static(fov=shading.get_fov(), isovalue=0.5)

    def set_static(self, fov, isovalue, lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
        """As ``SuperResolutionPipeline.set_static``."""
        r = self.renderer
        self._lookat = tuple(float(v) for v in fmt3(lookat).split(","))
        r.send_command("cameraLookAt", fmt3(lookat))
        r.send_command("cameraUp", fmt3(up))
        r.send_command("cameraFoV", "%.3f" % fov)
        r.send_command("isovalue", "%5.3f" % float(isovalue))
        r.send_command("aoradius", "%5.3f" % 0.01)
        r.send_command("aosamples", "0")
        r.send_command("resolution", "%d,%d" % (self.low_w, self.low_h))
        r.send_command("viewport", "%d,%d,%d,%d" % (0, 0, self.low_w, self.low_h))

    def reset(self, flush=True):
        self.previous = None

    def _drop_prefetched(self):
        pass
