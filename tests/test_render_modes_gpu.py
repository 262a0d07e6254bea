"""GPU: the viewer's non-network render modes -- the launch (``ops.display_baseline_frame`` / ``isrDisplayBaselineFrame``,
csrc/sr_display.hip) against its definition (``viewer.compose_baseline`` on the same device tensors), and ``viewer.DisplayStage`` in those
modes through the renderer's and the kernels' C-ABI.

Rule of every comparison, as in tests/test_display_gpu.py: ``torch.equal`` wherever no shading enters (the kernel performs the
definition's operations in the definition's order), 1e-4 wherever a shaded colour enters -- the colour view, whose colour is shaded at
the G-buffer's resolution and then interpolated (bicubic's absolute weight sum is 1.375^2 = 1.89: a shading difference is at most
doubled), and any focus window in it.  Measured maxima: profiles/render_modes.md."""
import argparse

import pytest
import torch

import render_scenes as S
import test_display_gpu as D
from isosurfacesuperresolution_amd import ops, viewer
from isosurfacesuperresolution_amd.pipeline import default_shading

pytestmark = pytest.mark.gpu

# a single row; a width below the four taps (every bicubic index clamps); W % 4 alignment of the bytes; width != height; odd sizes
SIZES = [(1, 9), (3, 2), (8, 8), (5, 64), (23, 37)]
MODES = viewer.BASELINE_MODES
SHADED = 1e-4


def both(h, w, mode, smoothing=0.0, focus=None, focus_gbuffer=None, uint8=False, **kw):
    """-> (launch, definition) on the random tensors of ``test_display_gpu.frame_inputs(h, w)``; ground truth takes the full-resolution
    buffer as its G-buffer."""
    x = D.frame_inputs(h, w)
    sh = default_shading("cuda", 30.0)
    g = x["full"] if mode == "ground_truth" else x["gbuffer"]
    common = dict(shading=sh, filled_flow=x["flow"], prev_displayed=x["prev"] if smoothing else None, post_smoothing=smoothing, focus=focus,
                  focus_gbuffer=(x["full"] if focus_gbuffer is None else focus_gbuffer) if focus is not None else None, **kw)
    out8 = torch.zeros((4 * h, 4 * w, 4), dtype=torch.uint8, device="cuda") if uint8 else None
    got = ops.display_baseline_frame(g, mode, out8=out8, **common)
    ref = viewer.compose_baseline(g, mode, present_uint8=uint8, **common)
    return ((got, out8), ref) if uint8 else (got, ref)


@pytest.mark.parametrize("h,w", SIZES)
def test_launch_is_bit_identical_to_the_definition_where_no_shading_enters(h, w):
    for mode in MODES:
        for channel in ("mask", "normal", "depth", "ao", "flow"):
            if mode == "ground_truth" and channel == "flow":
                with pytest.raises(ValueError):
                    both(h, w, mode, channel=channel)
                continue
            for smoothing in (0.0, 0.3, 1.0):
                got, ref = both(h, w, mode, channel=channel, smoothing=smoothing)
                assert got.shape == ref.shape == (1, 3, 4 * h, 4 * w)
                assert torch.equal(got, ref), (mode, channel, smoothing, (got - ref).abs().max().item())
    # the modes differ, and ground truth is not smoothed
    assert not torch.equal(both(h, w, "nearest", channel="ao")[0], both(h, w, "bicubic", channel="ao")[0])
    assert torch.equal(both(h, w, "ground_truth", channel="ao", smoothing=0.3)[0], both(h, w, "ground_truth", channel="ao")[0])


@pytest.mark.parametrize("h,w", SIZES)
def test_colour_view_agrees_with_the_definition(h, w):
    for mode in MODES:
        for smoothing in (0.0, 0.3):
            got, ref = both(h, w, mode, channel="color", smoothing=smoothing)
            dist = (got - ref).abs().max().item()
            print("colour %s %dx%d smoothing %.1f: launch vs definition %.2e" % (mode, h, w, smoothing, dist))
            assert dist <= SHADED, (mode, smoothing, dist)


def windows(H, W):
    """The four corners, and a window larger than the image."""
    win = max(2, min(H, W) // 3) + 1
    return {"corner00": ((1, 1), win, 2), "corner01": ((W - 2, 1), win, 2), "corner10": ((1, H - 2), win, 2),
            "corner11": ((W - 2, H - 2), win, 2), "everything": ((W // 2, H // 2), 4 * (H + W), H + W)}


@pytest.mark.parametrize("h,w", SIZES)
def test_focus_windows(h, w):
    H, W = 4 * h, 4 * w
    for name, (centre, win, blur) in windows(H, W).items():
        region = viewer.focus_region(H, W, centre, win, blur, device="cuda")
        covered = int((region[1] > 0).sum())
        assert covered > 0 and (name != "everything" or covered >= H * W - 1)
        for mode in ("nearest", "bilinear", "bicubic"):
            for cfg in (dict(channel="color"), dict(channel="color", smoothing=0.3)):
                got, ref = both(h, w, mode, focus=region, **cfg)
                dist = (got - ref).abs().max().item()
                print("%s %s %dx%d %s: launch vs definition %.2e" % (name, mode, h, w, cfg, dist))
                assert dist <= SHADED, (name, mode, cfg, dist)
                assert not torch.equal(got, both(h, w, mode, **cfg)[0])
            # the other views take the full-resolution buffer's channels as they are: no shading, the same bits
            for cfg in (dict(channel="mask"), dict(channel="normal", smoothing=0.3), dict(channel="depth"), dict(channel="ao", smoothing=1.0)):
                got, ref = both(h, w, mode, focus=region, **cfg)
                assert torch.equal(got, ref), (name, mode, cfg, (got - ref).abs().max().item())
        # ground truth shows no window
        assert torch.equal(both(h, w, "ground_truth", focus=region, channel="normal")[0], both(h, w, "ground_truth", channel="normal")[0])


@pytest.mark.parametrize("h,w", SIZES)
def test_nothing_outside_the_viewport_enters_the_arithmetic(h, w):
    H, W = 4 * h, 4 * w
    x = D.frame_inputs(h, w)
    for name in ("corner00", "corner11"):
        region = viewer.focus_region(H, W, *windows(H, W)[name], device="cuda")
        x0, y0, x1, y1 = region[0]
        poisoned = torch.full_like(x["full"], float("nan"))
        poisoned[y0:y1, x0:x1] = x["full"][y0:y1, x0:x1]
        for mode in ("nearest", "bilinear", "bicubic"):
            for cfg in (dict(channel="color"), dict(channel="mask"), dict(channel="depth", smoothing=0.3)):
                clean, _ = both(h, w, mode, focus=region, **cfg)
                got, ref = both(h, w, mode, focus=region, focus_gbuffer=poisoned, **cfg)
                assert torch.isfinite(got).all() and torch.equal(got, clean), (name, mode, cfg)
                assert torch.isfinite(ref).all()


@pytest.mark.parametrize("h,w", SIZES)
def test_eight_bit_output_equals_the_definitions(h, w):
    for mode in MODES:
        for cfg in (dict(channel="depth"), dict(channel="ao", smoothing=0.3), dict(channel="normal")):
            (got, got8), (ref, ref8) = both(h, w, mode, uint8=True, **cfg)
            assert torch.equal(got, ref) and got8.dtype == torch.uint8 and torch.equal(got8, ref8), (mode, cfg)
            assert torch.equal(got8, viewer.to_uint8(got)) and (got8[..., 3] == 255).all()
        (got, got8), _ = both(h, w, mode, uint8=True, channel="color", smoothing=0.3)
        assert torch.equal(got8, viewer.to_uint8(got))              # the bytes are the float image's, whatever the shading's last bit


def test_unsupported_arguments_raise():
    x = D.frame_inputs(8, 8)
    sh = default_shading("cuda", 30.0)
    g, flow, prev, full = x["gbuffer"], x["flow"], x["prev"], x["full"]
    region = viewer.focus_region(32, 32, (16, 16), 8, 2, device="cuda")
    call = ops.display_baseline_frame
    call(g, "bilinear", shading=sh)
    bad = [
        lambda: call(g.cpu(), "bilinear", shading=sh),                                            # device
        lambda: call(g.double(), "bilinear", shading=sh),                                         # dtype
        lambda: call(g[:, :, :11], "bilinear", shading=sh),                                       # shape
        lambda: call(g.permute(1, 0, 2), "bilinear", shading=sh),                                 # not contiguous
        lambda: call(full[:30], "ground_truth", shading=sh),                                      # ground truth is [4h, 4w, 12]
        lambda: call(g, "bilinear", shading=sh, out=torch.empty((1, 3, 32, 32), device="cuda").transpose(2, 3)),   # out not contiguous
        lambda: call(g, "bilinear", shading=sh, out=torch.empty((1, 3, 32, 31), device="cuda")),
        lambda: call(g, "bilinear", shading=sh, out8=torch.empty((32, 32, 3), dtype=torch.uint8, device="cuda")),
        lambda: call(g, "bilinear", shading=sh, filled_flow=flow, prev_displayed=prev, post_smoothing=0.5, out=prev),   # out is prev
        lambda: call(g, "bilinear", shading=sh, prev_displayed=prev, post_smoothing=0.5),         # smoothing without flow
        lambda: call(g, "bilinear", shading=sh, channel="flow"),                                  # flow view without flow
        lambda: call(g, "bilinear", shading=sh, filled_flow=flow[:, :1], channel="flow"),
        lambda: call(full, "ground_truth", shading=sh, filled_flow=flow, channel="flow"),         # no flow view in ground truth
        lambda: call(g, "bilinear", shading=sh, focus=region),                                    # window without its render
        lambda: call(g, "bilinear", shading=sh, focus=region, focus_gbuffer=full.cpu()),
        lambda: call(g, "bilinear", shading=sh, channel="depth", bounds=torch.zeros(2)),
        lambda: call(g, "bilinear", shading=sh, workspace=torch.empty((11, 8, 8), device="cuda")),
        lambda: call(g, "bilinear"),                                                              # the colour view needs the shading
        lambda: call(g, "cubic", shading=sh),
        lambda: call(g, "network", shading=sh),
        lambda: call(g, "bilinear", shading=sh, channel="colour"),
    ]
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail("case %d did not raise" % k)


def test_a_failing_launch_raises_runtime_error(monkeypatch):
    class Lib:
        @staticmethod
        def isrDisplayBaselineFrame(params, stream):
            return -2
    monkeypatch.setattr(ops, "_sr", lambda: Lib)
    with pytest.raises(RuntimeError):
        ops.display_baseline_frame(D.frame_inputs(8, 8)["gbuffer"], "nearest", channel="mask")


# ---- through the C-ABI: renderer + display stage -----------------------------------------------------------------------------------------
LOW, FOCUS, AO_SAMPLES = D.LOW, D.FOCUS, D.AO_SAMPLES
HIGH = (4 * LOW[0], 4 * LOW[1])


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
    D.run(scene, frames=2)            # the model's first frame settles the range guard's routing: every run below takes the same kernels
    return scene


def show(stage, plan):
    """``plan``: (mode, camera index) per frame.  Per frame, copies of what the stage displayed and of what it composed from."""
    record = []
    for mode, k in plan:
        stage.set_mode(mode)
        before = stage.previous
        result = stage.frame(stage_origins(stage)[k], stage_origins(stage)[k + 1])
        displayed, rgba = result if stage.present_uint8 else (result, None)
        record.append(dict(mode=mode, k=k, displayed=displayed.clone(), rgba=None if rgba is None else rgba.clone(),
                           gbuffer=stage._frame_state[0].clone(), before=None if before is None else before.clone()))
    torch.cuda.synchronize()
    return record


def stage_origins(stage):
    return stage._test_origins


def make_stage(scene, **kw):
    stage = D.make_stage(scene, **kw)
    stage._test_origins = scene[2]
    return stage


def plain_render(scene, origin, size, ao_samples, viewport=None):
    """A G-buffer [rows, cols, 12] of ``origin`` rendered here, outside any stage."""
    from isosurfacesuperresolution_amd.volumes import fmt3
    renderer = scene[0]
    out = torch.zeros((size[1], size[0], 12), dtype=torch.float32, device="cuda")
    for cmd, value in (("cameraOrigin", fmt3(origin)), ("resolution", "%d,%d" % size), ("viewport", "%d,%d,%d,%d" % (viewport or (0, 0) + size)),
                       ("aoradius", "%5.3f" % 0.01), ("aosamples", "%d" % ao_samples)):
        renderer.send_command(cmd, value)
    renderer.render_async(out, torch.cuda.current_stream())
    renderer.send_command("aosamples", "0")
    torch.cuda.synchronize()
    return out


def definition_of(scene, f, channel, region=None, smoothing=0.0):
    """``compose_baseline`` on a recorded frame's own tensors (the focus window rendered here)."""
    full = plain_render(scene, scene[2][f["k"]], HIGH, AO_SAMPLES, region[0]) if region is not None and f["mode"] != "ground_truth" else None
    flow = ops.fill_flow_gbuffer(f["gbuffer"]) if f["mode"] != "ground_truth" else None
    return viewer.compose_baseline(f["gbuffer"], f["mode"], default_shading("cuda", 30.0), filled_flow=flow, channel=channel, focus=region,
                                   focus_gbuffer=full, prev_displayed=f["before"], post_smoothing=smoothing, present_uint8=True)


@pytest.mark.parametrize("channel", viewer.CHANNELS)
@pytest.mark.parametrize("mode", MODES)
def test_stage_frame_equals_the_definition_on_the_stages_own_tensors(scene, mode, channel):
    kw = dict(channel=channel, masking=True, post_smoothing=0.3, focus=FOCUS, focus_ao_samples=AO_SAMPLES, ao_samples=AO_SAMPLES,
              present_uint8=True, mode=mode)
    stage = make_stage(scene, **kw)
    if mode == "ground_truth" and channel == "flow":
        with pytest.raises(ValueError):
            stage.frame(scene[2][0])
        return
    record = show(stage, [(mode, 0), (mode, 1), (mode, 2)])
    assert stage.pipeline.previous is None
    region = viewer.focus_region(HIGH[1], HIGH[0], *FOCUS, device="cuda")
    rows = HIGH[1] if mode == "ground_truth" else LOW[1]
    for f in record:
        assert f["gbuffer"].shape[0] == rows and (f["gbuffer"][..., 3] > 0).any() and torch.isfinite(f["gbuffer"]).all()
        ref, ref8 = definition_of(scene, f, channel, region, 0.3)
        dist = (f["displayed"] - ref).abs().max().item()
        print("%s %s frame %d: stage vs definition %.2e" % (mode, channel, f["k"], dist))
        if channel != "color":
            assert torch.equal(f["displayed"], ref) and torch.equal(f["rgba"], ref8), (f["k"], dist)
        else:
            assert dist <= SHADED, (f["k"], dist)
            assert (f["rgba"].int() - ref8.int()).abs().max().item() <= 1
    assert not torch.equal(record[1]["displayed"], record[0]["displayed"])


def test_ground_truth_frame_is_the_full_resolution_render(scene):
    stage = make_stage(scene, mode="ground_truth", channel="normal", ao_samples=AO_SAMPLES)
    f = show(stage, [("ground_truth", 1)])[0]
    scene[0].set_last_camera(scene[2][0])                        # the flow reference make_stage starts from
    full = plain_render(scene, scene[2][1], HIGH, AO_SAMPLES)
    assert tuple(f["gbuffer"].shape) == (HIGH[1], HIGH[0], 12) and torch.equal(f["gbuffer"], full)
    assert torch.equal(f["displayed"], viewer.compose_baseline(full, "ground_truth", default_shading("cuda", 30.0), channel="normal"))
    # ... and it is not the low-resolution render resized
    low = plain_render(scene, scene[2][1], LOW, AO_SAMPLES)
    assert not torch.equal(f["displayed"], viewer.compose_baseline(low, "bicubic", default_shading("cuda", 30.0), channel="normal"))


def test_a_baseline_frame_restarts_the_networks_recurrence(scene):
    """network -> bilinear -> network: the last frame is the first frame of a sequence -- that of a stage that was ``reset()`` there."""
    o = scene[2]
    a = make_stage(scene, ao_samples=AO_SAMPLES)
    a.frame(o[0], o[1])                                           # (the next frame is rendered ahead, without AO: dropped below)
    a.set_mode("bilinear")
    middle = a.frame(o[1]).clone()
    assert a.pipeline.previous is None and a.pipeline._prefetched is None
    a.set_mode("network")
    last = a.frame(o[2], o[3]).clone()
    last_gbuffer = a.pipeline.gbuffer.clone()
    b = make_stage(scene)
    first = b.frame(o[0], o[1]).clone()
    b.reset()
    torch.cuda.synchronize()                                      # (the frame rendered ahead is dropped: let it finish first)
    from isosurfacesuperresolution_amd.volumes import fmt3
    scene[0].set_last_camera(tuple(float(v) for v in fmt3(o[1]).split(",")))   # frame 2's flow is measured against the displayed frame 1, as the renderer parsed it
    again = b.frame(o[2], o[3]).clone()
    torch.cuda.synchronize()
    assert torch.equal(last, again) and not torch.equal(last, first) and not torch.equal(middle, last)
    assert torch.equal(last_gbuffer, b.pipeline.gbuffer)          # AO parameters, resolution and flow reference were put back
    assert last_gbuffer[..., 8:10].abs().max().item() > 0


def test_displayed_image_advances_in_every_mode_and_ground_truth_is_not_smoothed(scene):
    stage = make_stage(scene, mode="bilinear", channel="normal", post_smoothing=0.5, ao_samples=AO_SAMPLES)
    record = show(stage, [("bilinear", 0), ("ground_truth", 1), ("bilinear", 2)])
    truth, after = record[1], record[2]
    assert truth["before"] is not None and torch.equal(truth["before"], record[0]["displayed"])
    assert torch.equal(truth["displayed"], definition_of(scene, truth, "normal", None, 0.0)[0])      # not smoothed
    assert torch.equal(after["before"], truth["displayed"])                                          # ... but it is the next "previous"
    assert torch.equal(after["displayed"], definition_of(scene, after, "normal", None, 0.5)[0])
    unsmoothed = dict(after, before=None)
    assert not torch.equal(after["displayed"], definition_of(scene, unsmoothed, "normal", None, 0.0)[0])


def test_flow_is_measured_against_the_frame_displayed_before_whichever_mode_showed_it(scene):
    """baseline, its focus render, ground truth, baseline: neither the window's render nor the mode in between moves the flow reference
    anywhere but to the displayed cameras."""
    o = scene[2]
    stage = make_stage(scene, mode="nearest", focus=FOCUS, focus_ao_samples=AO_SAMPLES, ao_samples=AO_SAMPLES)
    record = show(stage, [("nearest", 0), ("ground_truth", 1), ("nearest", 2)])
    scene[0].set_last_camera(o[0])
    plain0 = plain_render(scene, o[0], LOW, AO_SAMPLES)
    plain1 = plain_render(scene, o[1], HIGH, AO_SAMPLES)
    plain2 = plain_render(scene, o[2], LOW, AO_SAMPLES)
    assert plain2[..., 8:10].abs().max().item() > 0 and plain1[..., 8:10].abs().max().item() > 0
    for f, plain in zip(record, (plain0, plain1, plain2)):
        assert torch.equal(f["gbuffer"][..., 8:10], plain[..., 8:10]), f["k"]
        assert torch.equal(f["gbuffer"], plain), f["k"]


def counted(renderer, monkeypatch):
    calls = []
    real = renderer.render_async
    monkeypatch.setattr(renderer, "render_async", lambda tensor, stream=None: (calls.append(tuple(tensor.shape)), real(tensor, stream))[1])
    return calls


def test_refocus_in_a_baseline_mode_renders_the_window_only_and_moves_no_state(scene, monkeypatch):
    stage = make_stage(scene, mode="bicubic", post_smoothing=0.3, ao_samples=AO_SAMPLES, focus_ao_samples=AO_SAMPLES)
    record = show(stage, [("bicubic", 0), ("bicubic", 1)])
    state, state_values = stage.previous, stage.previous.clone()
    calls = counted(scene[0], monkeypatch)
    plain = stage.refocus(None).clone()
    assert calls == [] and torch.equal(plain, record[-1]["displayed"])       # no window: the frame as it was displayed, nothing rendered
    focused = stage.refocus(FOCUS).clone()
    assert calls == [(HIGH[1], HIGH[0], 12)]                                 # the window, and no low-resolution frame
    region = viewer.focus_region(stage.H, stage.W, *FOCUS, device="cuda")
    changed = (focused != plain).any(dim=1)
    assert changed.any() and not (changed & ~(region[1] > 0)).any()
    assert stage.previous is state and torch.equal(stage.previous, state_values)
    # the sequence goes on as if nobody had looked
    stage.set_focus(None)
    nxt = stage.frame(scene[2][2]).clone()
    straight = show(make_stage(scene, mode="bicubic", post_smoothing=0.3, ao_samples=AO_SAMPLES), [("bicubic", 0), ("bicubic", 1), ("bicubic", 2)])
    assert torch.equal(nxt, straight[2]["displayed"])


def test_refocus_in_ground_truth_mode_returns_the_stored_image(scene, monkeypatch):
    stage = make_stage(scene, mode="ground_truth", ao_samples=AO_SAMPLES)
    record = show(stage, [("ground_truth", 1)])
    calls = counted(scene[0], monkeypatch)
    assert torch.equal(stage.refocus(FOCUS), record[0]["displayed"]) and calls == []


def test_render_only_runs_the_four_modes_without_a_model(scene):
    renderer, _, origins = scene
    sh = default_shading("cuda", 30.0)
    pipe = viewer.RenderOnly(renderer, sh, LOW)
    pipe.set_static(fov=30.0, isovalue=0.5)
    with pytest.raises(ValueError):
        viewer.DisplayStage(pipe)
    with pytest.raises(ValueError):
        viewer.DisplayStage(pipe, mode="network")
    stage = viewer.DisplayStage(pipe, mode="nearest", channel="normal", post_smoothing=0.3, ao_samples=AO_SAMPLES, present_uint8=True)
    stage._test_origins = origins
    with pytest.raises(ValueError):
        stage.set_mode("network")
    renderer.set_last_camera(origins[0])
    record = show(stage, [(m, k) for k, m in enumerate(MODES)])
    for f in record:
        ref, ref8 = definition_of(scene, f, "normal", None, 0.3)
        assert torch.equal(f["displayed"], ref) and torch.equal(f["rgba"], ref8), f["mode"]
    # the same frames as a stage around a pipeline with a model shows in these modes
    other = show(make_stage(scene, mode="nearest", channel="normal", post_smoothing=0.3, ao_samples=AO_SAMPLES, present_uint8=True),
                 [(m, k) for k, m in enumerate(MODES)])
    for f, g in zip(record, other):
        assert torch.equal(f["displayed"], g["displayed"]), f["mode"]


@pytest.mark.parametrize("mode", MODES)
def test_module_path_stage_matches_the_launch(scene, mode):
    """``fused=False`` composes with ``compose_baseline``: the same bits where no shading enters, 1e-4 in the colour view."""
    plan = [(mode, 0), (mode, 1), (mode, 2)]
    for channel in ("depth", "color"):
        kw = dict(mode=mode, channel=channel, post_smoothing=0.3, ao_samples=AO_SAMPLES)
        a, b = show(make_stage(scene, **kw), plan), show(make_stage(scene, fused=False, **kw), plan)
        for fa, fb in zip(a, b):
            assert torch.equal(fa["gbuffer"], fb["gbuffer"])
            dist = (fa["displayed"] - fb["displayed"]).abs().max().item()
            assert torch.equal(fa["displayed"], fb["displayed"]) if channel == "depth" else dist <= SHADED, (channel, fa["k"], dist)
