"""GPU: the display stage's launch (``ops.display_frame`` / ``isrDisplayFrame``, csrc/sr_display.hip) against its definition
(``viewer.compose_display`` on the same device tensors), and ``viewer.DisplayStage`` through the renderer's and the kernels' C-ABI.

Rule of every comparison: ``torch.equal`` wherever no shading enters (the kernel performs the definition's operations in the definition's
order), 1e-4 wherever the focus window is shaded (the tolerance ``finish_frame`` has against the module path)."""
import argparse
import functools

import pytest
import torch

import render_scenes as S
from isosurfacesuperresolution_amd import ops, viewer
from isosurfacesuperresolution_amd.pipeline import default_shading

pytestmark = pytest.mark.gpu

SIZES = [(23, 37), (8, 8), (5, 64), (1, 9)]        # odd sizes, a single row, width != height: swapped strides or taps show
SHADED = 1e-4


@functools.lru_cache(maxsize=None)
def frame_inputs(h, w):
    """Random tensors of one frame, as in test_fused_frame_kernels_match_module_path; made once per size and left unchanged."""
    gen = torch.Generator(device="cpu").manual_seed(100 * h + w)
    r = lambda *shape: torch.rand(*shape, generator=gen)
    H, W = 4 * h, 4 * w
    g = r(h, w, 12)
    g[..., 3] = (g[..., 3] > 0.4).float()
    g[..., 7] = g[..., 7] * g[..., 3]                       # depth 0 in the background: the (d <= 1e-5) term of the bounds acts
    g[..., 8:10] = (g[..., 8:10] - 0.5) * 0.05
    n = r(1, 3, H, W) * 2 - 1
    raw = torch.cat([r(1, 1, H, W) * 2 - 1, n / n.norm(dim=1, keepdim=True).clamp_min(1e-7), r(1, 2, H, W)], dim=1)
    full = r(H, W, 12)
    full[..., 3] = (full[..., 3] > 0.4).float()
    full[..., 4:7] = full[..., 4:7] * 2 - 1
    d = dict(gbuffer=g, rgb=r(1, 3, H, W), raw=raw, flow=(r(1, 2, h, w) - 0.5) * 0.05, prev=r(1, 3, H, W), full=full)
    return {k: v.cuda().contiguous() for k, v in d.items()}


def both(h, w, raw=True, smoothing=0.0, focus=None, focus_gbuffer=None, uint8=False, **kw):
    """-> (kernel, definition) on the inputs of ``frame_inputs(h, w)``."""
    x = frame_inputs(h, w)
    sh = default_shading("cuda", 30.0)
    args = (x["gbuffer"], x["rgb"], x["raw"] if raw else None, x["flow"])
    common = dict(shading=sh, background0=1.0, prev_displayed=x["prev"] if smoothing else None, post_smoothing=smoothing, focus=focus,
                  focus_gbuffer=(x["full"] if focus_gbuffer is None else focus_gbuffer) if focus is not None else None, **kw)
    out8 = torch.zeros((4 * h, 4 * w, 4), dtype=torch.uint8, device="cuda") if uint8 else None
    got = ops.display_frame(*args, out8=out8, **common)
    ref = viewer.compose_display(*args, present_uint8=uint8, **common)
    return ((got, out8), ref) if uint8 else (got, ref)


UNSHADED_CONFIGS = [dict(channel="color", smoothing=0.3), dict(channel="color", smoothing=1.0), dict(channel="flow"),
                    dict(channel="flow", smoothing=0.3), dict(channel="mask"), dict(channel="normal"), dict(channel="depth"), dict(channel="ao"),
                    dict(channel="color", masking=True), dict(channel="mask", masking=True), dict(channel="normal", masking=True, smoothing=0.3),
                    dict(channel="depth", masking=True), dict(channel="ao", masking=True)]


@pytest.mark.parametrize("h,w", SIZES)
def test_kernel_is_bit_identical_to_the_definition_where_no_shading_enters(h, w):
    for cfg in UNSHADED_CONFIGS:
        for raw in (True, False):                    # the unshaded networks' route, and a colour network's (raw None, three-channel rgb)
            got, ref = both(h, w, raw=raw, **cfg)
            assert got.shape == ref.shape == (1, 3, 4 * h, 4 * w)
            assert torch.equal(got, ref), (cfg, raw, (got - ref).abs().max().item())


def windows(H, W):
    win = max(2, min(H, W) // 3)
    return {"inside": ((W // 2, H // 2), win, max(1, win // 2)), "corner": ((1, H - 1), win + 1, 2), "everything": ((W // 2, H // 2), 4 * (H + W), H + W),
            "hard_edge": ((W // 3, H // 2), win, 0), "nothing": ((-50, -70), 10, 4)}


@pytest.mark.parametrize("h,w", SIZES)
def test_focus_windows(h, w):
    H, W = 4 * h, 4 * w
    for name, (centre, win, blur) in windows(H, W).items():
        region = viewer.focus_region(H, W, centre, win, blur, device="cuda")
        covered = int((region[1] > 0).sum())
        assert (covered == 0) == (name == "nothing") and (name != "everything" or covered >= H * W - 1)
        for cfg in (dict(channel="color"), dict(channel="color", masking=True, smoothing=0.3), dict(channel="color", raw=False)):
            got, ref = both(h, w, focus=region, **cfg)
            dist = (got - ref).abs().max().item()
            print("%s %dx%d %s: kernel vs definition %.2e" % (name, h, w, cfg, dist))
            assert dist <= SHADED, (name, cfg, dist)
            if name == "nothing":
                assert torch.equal(got, both(h, w, **cfg)[0])
        # the other views take the full-resolution buffer's channels as they are: no shading, the same bits
        for cfg in (dict(channel="mask"), dict(channel="normal", masking=True), dict(channel="depth", smoothing=0.3), dict(channel="ao", raw=False)):
            got, ref = both(h, w, focus=region, **cfg)
            assert torch.equal(got, ref), (name, cfg, (got - ref).abs().max().item())


@pytest.mark.parametrize("h,w", SIZES)
def test_nothing_outside_the_viewport_enters_the_arithmetic(h, w):
    H, W = 4 * h, 4 * w
    x = frame_inputs(h, w)
    for name in ("inside", "corner", "nothing"):
        region = viewer.focus_region(H, W, *windows(H, W)[name], device="cuda")
        x0, y0, x1, y1 = region[0]
        poisoned = torch.full_like(x["full"], float("nan"))
        poisoned[y0:y1, x0:x1] = x["full"][y0:y1, x0:x1]
        for cfg in (dict(channel="color"), dict(channel="mask"), dict(channel="depth", masking=True)):
            clean, _ = both(h, w, focus=region, **cfg)
            got, ref = both(h, w, focus=region, focus_gbuffer=poisoned, **cfg)
            assert torch.isfinite(got).all() and torch.equal(got, clean), (name, cfg)
            assert torch.isfinite(ref).all()


@pytest.mark.parametrize("h,w", SIZES)
def test_eight_bit_output_equals_the_definitions(h, w):
    for cfg in (dict(channel="color", smoothing=0.3), dict(channel="depth"), dict(channel="flow"), dict(channel="color", raw=False, masking=True)):
        (got, got8), (ref, ref8) = both(h, w, uint8=True, **cfg)
        assert torch.equal(got, ref) and got8.dtype == torch.uint8 and torch.equal(got8, ref8), cfg
        assert (got8[..., 3] == 255).all()


def test_unsupported_arguments_raise():
    x = frame_inputs(8, 8)
    assert ops.display_supported(x["gbuffer"], x["rgb"], x["raw"]) and not ops.display_supported(x["gbuffer"].cpu(), x["rgb"].cpu())
    assert not ops.display_supported(x["gbuffer"], x["rgb"][:, :, :-1])
    with pytest.raises(ValueError):
        ops.display_frame(x["gbuffer"].cpu(), x["rgb"].cpu())
    with pytest.raises(ValueError):
        ops.display_frame(x["gbuffer"], x["rgb"], x["raw"], x["flow"], prev_displayed=x["prev"], post_smoothing=0.5, out=x["prev"])
    with pytest.raises(ValueError):
        ops.display_frame(x["gbuffer"], x["rgb"], x["raw"], None, channel="flow")
    with pytest.raises(ValueError):
        ops.display_frame(x["gbuffer"], x["rgb"], x["raw"], channel="colour")


# ---- through the C-ABI: renderer + network + display stage -----------------------------------------------------------------------------
LOW = (48, 32)                      # (width, height): 192 x 128 displayed
FOCUS = ((80, 60), 30, 10)
AO_SAMPLES = 4


@pytest.fixture(scope="module")
def scene():
    from isosurfacesuperresolution_amd import models, volumes as V
    from isosurfacesuperresolution_amd.inference import DirectRenderer, LoadedModel
    opt = argparse.Namespace(upsample='bilinear', reconType='residual', useBN=False, numResidualLayers=10)
    torch.manual_seed(5)
    net = models.createNetwork('EnhanceNet', 4, 101, [0, 1, 2, 3, 4], 6, opt)
    model = LoadedModel.from_model(net, "cuda", parameters={"initialImage": "zero"})
    renderer = DirectRenderer()
    renderer.load_dense(S.soft_spheres((32, 32, 32), [((15.5, 15.5, 15.5), 9.0)], 1e-3))
    scene = renderer, model, [V.orbit_camera(k) for k in range(6)]
    run(scene, frames=2)              # the model's first frame settles the range guard's routing: every run below takes the same kernels
    return scene


def make_stage(scene, **kw):
    from isosurfacesuperresolution_amd.pipeline import SuperResolutionPipeline
    renderer, model, origins = scene
    pipe = SuperResolutionPipeline(renderer, model, default_shading("cuda", 30.0), LOW, graph=False)
    pipe.set_static(fov=30.0, isovalue=0.5)
    renderer.set_last_camera(origins[0])                 # every run starts from the same flow reference
    return viewer.DisplayStage(pipe, **kw)


def run(scene, frames=5, **kw):
    """A five-frame orbit with the next camera given (the next render is in flight while the stage works); per frame, copies of what the
    stage displayed and of everything it composed from."""
    origins = scene[2]
    stage = make_stage(scene, **kw)
    pipe = stage.pipeline
    record = []
    for k in range(frames):
        before = stage.previous
        result = stage.frame(origins[k], origins[k + 1])
        displayed, rgba = result if stage.present_uint8 else (result, None)
        gbuffer, rgb, raw, flow, bounds, _ = stage._frame_state
        record.append(dict(displayed=displayed.clone(), rgba=None if rgba is None else rgba.clone(), gbuffer=gbuffer.clone(), rgb=rgb.clone(),
                           raw=raw.clone(), flow=ops.fill_flow_gbuffer(gbuffer).clone(), used_flow=None if flow is None else flow.clone(),
                           before=None if before is None else before.clone()))
    torch.cuda.synchronize()
    return stage, record


def render_focus_separately(scene, origin, region):
    """The full-resolution G-buffer of the focus window, rendered here with the parameters the stage uses."""
    from isosurfacesuperresolution_amd.volumes import fmt3
    renderer = scene[0]
    H, W = 4 * LOW[1], 4 * LOW[0]
    out = torch.zeros((H, W, 12), dtype=torch.float32, device="cuda")
    for cmd, value in (("cameraOrigin", fmt3(origin)), ("resolution", "%d,%d" % (W, H)), ("viewport", "%d,%d,%d,%d" % region[0]),
                       ("aoradius", "%5.3f" % 0.01), ("aosamples", "%d" % AO_SAMPLES)):
        renderer.send_command(cmd, value)
    renderer.render_async(out, torch.cuda.current_stream())
    renderer.send_command("aosamples", "0")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("channel,exact", [("color", False), ("normal", True)])
def test_stage_frame_equals_the_definition_on_the_pipelines_own_tensors(scene, channel, exact):
    kw = dict(channel=channel, masking=True, post_smoothing=0.3, focus=FOCUS, focus_ao_samples=AO_SAMPLES, present_uint8=True)
    stage, record = run(scene, **kw)
    region = viewer.focus_region(4 * LOW[1], 4 * LOW[0], *FOCUS, device="cuda")
    sh = default_shading("cuda", 30.0)
    for k, f in enumerate(record):
        if f["used_flow"] is not None:
            assert torch.equal(f["used_flow"], f["flow"])            # the prefetched frame's fill is the frame's fill
        full = render_focus_separately(scene, scene[2][k], region)
        assert (full[..., 3] > 0).any() and torch.isfinite(full).all()       # the window sees the surface (a convex one: its ray-cast AO is 1)
        ref, ref8 = viewer.compose_display(f["gbuffer"], f["rgb"], f["raw"], f["flow"], shading=sh, channel=channel, masking=True, background0=1.0,
                                           focus=region, focus_gbuffer=full, prev_displayed=f["before"], post_smoothing=0.3, present_uint8=True)
        dist = (f["displayed"] - ref).abs().max().item()
        print("frame %d %s: stage vs definition %.2e" % (k, channel, dist))
        if exact:
            assert torch.equal(f["displayed"], ref) and torch.equal(f["rgba"], ref8), (k, dist)
        else:
            assert dist <= SHADED, (k, dist)
            assert (f["rgba"].int() - ref8.int()).abs().max().item() <= 1
        assert k == 0 or not torch.equal(f["displayed"], record[k - 1]["displayed"])


def test_focus_render_leaves_the_flow_reference_of_the_prefetched_frames_alone(scene):
    """The last-camera restore: with the next frame's render already in flight, the focus render of frame t must not become what frame
    t + 2's flow is measured against."""
    _, with_focus = run(scene, focus=FOCUS, focus_ao_samples=AO_SAMPLES, post_smoothing=0.3)
    _, without = run(scene, post_smoothing=0.3)
    assert with_focus[2]["gbuffer"][..., 8:10].abs().max().item() > 0      # there is a flow to get wrong
    for k, (a, b) in enumerate(zip(with_focus, without)):
        assert torch.equal(a["gbuffer"], b["gbuffer"]), k
        assert torch.equal(a["flow"], b["flow"]), k


def test_refocus_recomposes_the_stored_frame_and_moves_no_state(scene):
    stage, record = run(scene, frames=3, post_smoothing=0.3)
    pipe = stage.pipeline
    state, state_values = stage.previous, stage.previous.clone()
    network_state, network_values = pipe.previous, pipe.previous.clone()
    plain = stage.refocus(None).clone()
    assert torch.equal(plain, record[-1]["displayed"])                     # no window: the frame as it was displayed
    region = viewer.focus_region(stage.H, stage.W, *FOCUS, device="cuda")
    focused = stage.refocus(FOCUS).clone()
    changed = (focused != plain).any(dim=1)
    assert changed.any() and not (changed & ~(region[1] > 0)).any()        # only pixels with m > 0
    assert stage.previous is state and torch.equal(stage.previous, state_values)
    assert pipe.previous is network_state and torch.equal(pipe.previous, network_values)
    # ... and the sequence goes on as if nobody had looked: frame 3 equals the one of a run without the refocus
    stage.set_focus(None)
    nxt = stage.frame(scene[2][3], scene[2][4]).clone()
    _, straight = run(scene, frames=4, post_smoothing=0.3)
    assert torch.equal(nxt, straight[3]["displayed"])


def test_reset_starts_over(scene):
    """After ``reset()`` the next frame is a fresh stage's first frame."""
    stage, record = run(scene, frames=2, post_smoothing=0.5, focus=FOCUS)
    stage.reset()
    assert stage.previous is None and stage.pipeline.previous is None
    scene[0].set_last_camera(scene[2][0])
    again = stage.frame(scene[2][0], scene[2][1]).clone()
    _, fresh = run(scene, frames=1, post_smoothing=0.5, focus=FOCUS)
    assert torch.equal(again, fresh[0]["displayed"]) and not torch.equal(again, record[1]["displayed"])


def test_a_graph_pipeline_is_refused(scene):
    from isosurfacesuperresolution_amd.pipeline import SuperResolutionPipeline
    renderer, model, _ = scene
    pipe = SuperResolutionPipeline(renderer, model, default_shading("cuda", 30.0), LOW, graph=True)
    assert pipe.graph
    with pytest.raises(NotImplementedError):
        viewer.DisplayStage(pipe)
    pipe.close()


def test_module_path_stage_matches_the_launch(scene):
    """``fused=False`` composes with ``compose_display``: the same displayed images (no focus: the same bits)."""
    _, a = run(scene, frames=3, post_smoothing=0.3, channel="depth", masking=True)
    _, b = run(scene, frames=3, post_smoothing=0.3, channel="depth", masking=True, fused=False)
    for fa, fb in zip(a, b):
        assert torch.equal(fa["displayed"], fb["displayed"])
