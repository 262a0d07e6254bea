"""GPU: the two ends of an inference frame against the fp64 definition of tests/frame_boundary_common.py.

* finishing (csrc/sr_finish.h, inlined into ``finish_frame_kernel``, the small-Cout last layer and the tail forms): every entry point with
  every entry of ``SHADERS`` -- coloured vectors, a light that makes l.n change sign, both values of ``inverse_ao``, AO strengths 0 / 0.35 / 1,
  specular off, exponents 1 and 50, no shading -- at a single pixel, one tile, a width below one quad and ragged sizes;
* input assembly (csrc/sr_frame.hip): whole frame, ``rows=``, ``rows=`` + ``cols=`` and the packed form, crossed with the first-frame
  modes, ``ao_inverted`` and a previous frame, and a warp whose samples leave the previous frame on every side;
* ``aoInverted`` through ``SuperResolutionPipeline`` on its default fused route, eagerly and as a captured graph.

Bars (none of them from what the kernels give): per output tensor 4 x the fp32 module path's own distance from fp64 on the same inputs
+ the derived term for the kernel's power by repeated multiplication + 2^-22, + for the fused entry points the convolutions' share as
tests/test_tail_gpu.py states it.  Every figure is printed before it is asserted."""
import argparse
import ctypes
import functools

import pytest
import torch

import frame_boundary_common as C

pytestmark = pytest.mark.gpu
OPT = argparse.Namespace(upsample='bilinear', reconType='residual', useBN=False, numResidualLayers=10)


# ---- part 2: finishing ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _finish_cuda(h, w):
    return tuple(t.cuda() for t in C.finish_case(h, w))


@functools.lru_cache(maxsize=None)
def _fused_cuda(h, w):
    """The fused entries' operands on the device, once per size (the weight images are cached per tensor object)."""
    c = C.fused_case(h, w)
    return {k: c[k].cuda().contiguous() for k in ("f4", "w6", "b6", "w8", "b8", "x", "f6")}


def _run(entry, h, w, shader):
    """One launch of an entry point with one entry of SHADERS -> (next_prev, rgb or None)."""
    from isosurfacesuperresolution_amd import ops
    sh = C.make_shader(C.SHADERS[shader], "cuda")
    if entry == "finish_frame":
        raw, x = _finish_cuda(h, w)
        return ops.finish_frame(raw, x, sh)
    c = _fused_cuda(h, w)
    if entry == "final_conv_finish":
        return ops.final_conv_finish(c["f6"], c["w8"], c["b8"], c["x"], sh)
    assert ops.tail_supported(c["f4"], c["w6"], c["w8"])
    features = ops.pack_split(c["f4"]) if entry == "tail_packed" else c["f4"]
    return ops.tail_conv_finish(features, c["w6"], c["b6"], c["w8"], c["b8"], c["x"], sh)


def _reference(entry, h, w, shader):
    return C.reference("tail_f32" if entry == "tail_packed" else entry, h, w, shader)      # the packed units stand for the same fp32 features


def _compare(label, entry, h, w, shader, got):
    """Prints measured error and bar of both output tensors, -> [(what, error, bar)]."""
    ref = _reference(entry, h, w, shader)
    nxt, rgb = got
    assert (rgb is None) == (C.SHADERS[shader] is None)
    assert torch.isfinite(nxt).all() and (rgb is None or torch.isfinite(rgb).all())
    rows = [("next_prev", (nxt.double().cpu() - ref["next"]).abs().max().item(), ref["bar_next"])]
    if rgb is not None:
        rows.append(("rgb", (rgb.double().cpu() - ref["rgb"]).abs().max().item(), ref["bar_rgb"]))
    for what, err, bar in rows:
        print("%s %dx%d %s %s: |HIP - fp64| %.3e bar %.3e ratio %.3f (fp32 module path: %.3e)" % (
            label, h, w, shader, what, err, bar, err / bar, ref["err32_next" if what == "next_prev" else "err32_rgb"]))
    return [(shader, what, err, bar) for what, err, bar in rows]


def _assert_within(rows, label):
    worst = max(rows, key=lambda r: r[2] / r[3])
    print("%s: largest error / bar %.3f (%s %s)" % (label, worst[2] / worst[3], worst[0], worst[1]))
    for shader, what, err, bar in rows:
        assert err <= bar, "%s %s %s: |HIP - fp64| %.3e > bar %.3e" % (label, shader, what, err, bar)


@pytest.mark.parametrize("h,w", C.FINISH_SIZES)
@pytest.mark.parametrize("entry", C.ENTRY_POINTS)
def test_finishing_entry_point_with_every_shader_against_fp64(entry, h, w):
    """isrFinishFrame, isrConvSmallFinishFrame, isrConvTailFinishFrame and its Packed entry (default form), each filling its own
    parameter block from every option set; no pixel is excluded."""
    with torch.no_grad():
        got = {name: _run(entry, h, w, name) for name in C.SHADERS}
    torch.cuda.synchronize()
    rows = []
    for name in C.SHADERS:
        rows += _compare(entry, entry, h, w, name, got[name])
    _assert_within(rows, "%s %dx%d" % (entry, h, w))
    # without shading: no rgb, and the frame that is fed back is the shaded call's, bit for bit
    assert got["none"][1] is None
    for name in C.SHADED:
        assert torch.equal(got["none"][0], got[name][0]), name
    # the option is live: the two values of inverse_ao give different images
    a, b = (got[k][1] for k in C.INVERTED_PAIR)
    assert (a - b).abs().max().item() > 1e-2


@pytest.mark.parametrize("h,w", C.FINISH_SIZES)
def test_every_tail_form_with_the_inverted_coloured_shader(h, w, diag_lib):
    """The forms only ``isrDebugSetTailFused`` selects inline the finishing into kernels of their own (the in-kernel finish and the seam
    kernel of form 1, the combine kernel of form 0, the V form's finish): each with a non-default parameter block, fp32 and packed input."""
    from isosurfacesuperresolution_amd import ops
    lib = diag_lib
    lib.isrDebugSetTailFused.argtypes = [ctypes.c_int]
    got = {}
    try:
        for form in (0, 1, 2, 4):
            lib.isrDebugSetTailFused(form)
            with torch.no_grad():
                for entry in ("tail_f32", "tail_packed"):
                    if form == 1 and entry == "tail_packed":
                        continue                                       # (form 1 takes fp32 features only)
                    for name in C.INVERTED_PAIR:
                        got[(form, entry, name)] = _run(entry, h, w, name)
            torch.cuda.synchronize()
    finally:
        lib.isrDebugSetTailFused(2)
    rows = []
    for (form, entry, name), out in got.items():
        rows += _compare("%s form %d" % (entry, form), entry, h, w, name, out)
    _assert_within(rows, "tail forms %dx%d" % (h, w))
    for form, entry in {(f, e) for f, e, _ in got}:
        a, b = (got[(form, entry, k)] for k in C.INVERTED_PAIR)
        assert torch.equal(a[0], b[0]) and (a[1] - b[1]).abs().max().item() > 1e-2, (form, entry)
    assert not ops._sr().isrDebugTailState()


def test_display_stage_shades_the_focus_window_without_inverting():
    """The viewer's focus window is shaded non-inverted by design (its AO comes from the renderer; viewer.py): ``isrDisplayFrame`` has no
    such parameter, so a shader with ``inverse_ao`` set gives the same image."""
    from isosurfacesuperresolution_amd import ops, viewer
    h, w = 8, 12
    H, W = 4 * h, 4 * w
    g = torch.Generator().manual_seed(12)
    r = lambda *shape: torch.rand(*shape, generator=g)
    gb = r(h, w, 12)
    gb[..., 3] = (gb[..., 3] > 0.4).float()
    full = r(H, W, 12)
    full[..., 3] = (full[..., 3] > 0.3).float()
    full[..., 4:7] = full[..., 4:7] * 2 - 1
    gb, full, rgb = gb.cuda(), full.cuda().contiguous(), r(1, 3, H, W).cuda()
    region = viewer.focus_region(H, W, (W // 2, H // 2), 16, 5, device="cuda")
    assert int((region[1] > 0).sum()) > 100
    out = {}
    for name in C.INVERTED_PAIR + ("coloured_ao1", "coloured_ao1_inverted"):
        out[name] = ops.display_frame(gb, rgb, None, None, shading=C.make_shader(C.SHADERS[name], "cuda"), focus=region, focus_gbuffer=full)
    torch.cuda.synchronize()
    assert torch.equal(out["coloured"], out["coloured_inverted"]) and torch.equal(out["coloured_ao1"], out["coloured_ao1_inverted"])
    assert not torch.equal(out["coloured"], out["coloured_ao1"]) and not torch.equal(out["coloured"], rgb)      # (the window is shaded, with the AO strength)


# ---- part 3: assembly -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _trunk_convs():
    from isosurfacesuperresolution_amd import models
    torch.manual_seed(3)
    net = models.createNetwork('EnhanceNet', 4, 101, [0, 1, 2, 3, 4], 6, OPT).cuda().eval()
    return net, net.trunk_convs()


def _check_forms(label, gb, flow, prev, mode, inv, expect, flat64, bar, packed):
    """The four forms of one case: the whole frame against the definition, the row / rectangle forms and the packed form against the
    whole frame, bit for bit; a sentinel shows what a partial launch leaves alone."""
    from isosurfacesuperresolution_amd import ops
    h, w = gb.shape[0], gb.shape[1]
    whole = ops.assemble_input(gb, flow, prev, mode, inv)
    got = whole.cpu()
    if bar == 0.0:
        assert torch.equal(got, expect), (label, (got - expect).abs().max().item())
    else:
        err = (got[:, 5:].double() - flat64).abs().max().item()
        print("%s: |HIP - fp64| %.3e bar %.3e ratio %.3f" % (label, err, bar, err / bar))
        assert torch.equal(got[:, :5], expect[:, :5]) and err <= bar, (label, err, bar)
    if prev is None and mode == "unshaded":
        assert float(got[0, 85:].unique()) == (0.0 if inv else 1.0)                       # AO: 0 when inverted, 1 otherwise
    for (a, b), cols in C.rectangles(h, w):
        out = torch.full((1, 101, h, w), C.SENTINEL, device="cuda")
        part = ops.assemble_input(gb, flow, prev, mode, inv, out=out, rows=(a, b), cols=cols)
        c0, c1 = (0, w) if cols is None else cols
        assert part is out and torch.equal(part[:, :, a:b, c0:c1], whole[:, :, a:b, c0:c1]), (label, (a, b), cols)
        outside = torch.ones((h, w), dtype=torch.bool, device="cuda")
        outside[a:b, c0:c1] = False
        assert bool((part[0][:, outside] == C.SENTINEL).all()), (label, (a, b), cols)
        assert not bool((part[:, :, a:b, c0:c1] == C.SENTINEL).any())
    if packed:
        _, convs = _trunk_convs()
        with torch.no_grad():
            f_ref = ops.trunk_dataflow(whole, convs).clone()
            xp = ops.assemble_input_packed(gb, flow, prev, convs, mode, inv)
            assert xp is not None and getattr(xp, '_isr_prepacked', None) is not None
            f = ops.trunk_dataflow(xp, convs).clone()
        torch.cuda.synchronize()
        ops.trunk_check()
        assert torch.equal(xp[:, :5], whole[:, :5]), label
        assert torch.equal(f, f_ref), (label, (f - f_ref).abs().max().item())
    return whole


def _packed_offered(h, w):
    from isosurfacesuperresolution_amd import ops
    with torch.no_grad():                                      # (inference: the dataflow trunk does not take a frame that asks for gradients)
        offered = ops.ASSEMBLE_PACKED and ops.trunk_supported(torch.empty((1, 101, h, w), device="cuda"), _trunk_convs()[1])
    if (h, w) in C.PACKED_REQUIRED:
        assert offered
    return offered


@pytest.mark.parametrize("h,w", C.ASSEMBLE_SIZES)
def test_assembly_forms_modes_and_ao_inverted(h, w):
    from isosurfacesuperresolution_amd import ops
    gb, prev = (t.cuda() for t in C.assemble_case(h, w))
    packed = _packed_offered(h, w)
    flow = ops.fill_flow_gbuffer(gb)
    with_prev, flow_ref = C.assemble_reference_with_previous(h, w)
    assert torch.equal(flow.cpu(), flow_ref)
    unshaded = {}
    for mode in C.MODES:
        for inv in (False, True):
            label = "%dx%d %s inverted=%s" % (h, w, mode, inv)
            # with a previous frame: the definition, bit for bit, whatever the first-frame options say
            _check_forms(label + " previous", gb, flow, prev, mode, inv, with_prev, None, 0.0, packed)
            expect, flat64, bar = C.assemble_reference_first_frame(h, w, mode, inv)
            unshaded[(mode, inv)] = _check_forms(label + " first", gb, None, None, mode, inv, expect, flat64, bar, packed)
    a, b = unshaded[("unshaded", False)], unshaded[("unshaded", True)]
    assert torch.equal(a[:, :85], b[:, :85]) and float((a[:, 85:] - b[:, 85:]).abs().min()) == 1.0     # the flag moves the AO planes, and only them
    for mode in ("zero", "input"):
        assert torch.equal(unshaded[(mode, False)], unshaded[(mode, True)])


@pytest.mark.parametrize("h,w", C.LARGE_FLOW_SIZES)
def test_warp_with_samples_far_outside_the_previous_frame(h, w):
    """Flows of +-1.5 in normalised units on a third of the pixels and whole-pixel displacements on another third: quads of samples fall
    left, right, above and below the previous frame (the clamps that keep them addressable run everywhere, not only at the border), and
    the kernel still writes the definition's bits."""
    from isosurfacesuperresolution_amd import ops
    cover = C.warp_coverage(h, w, True)
    print((h, w), cover)
    assert cover["outside"] >= 0.10 and cover["inside"] >= 0.10 and all(cover["sides"])
    gb, prev = (t.cuda() for t in C.assemble_case(h, w, True))
    flow = ops.fill_flow_gbuffer(gb)
    expect, flow_ref = C.assemble_reference_with_previous(h, w, True)
    assert torch.equal(flow.cpu(), flow_ref) and float(flow_ref.abs().max()) == 1.5
    whole = _check_forms("%dx%d large flow" % (h, w), gb, flow, prev, "zero", True, expect, None, 0.0, _packed_offered(h, w))
    flat = whole[:, 5:]
    assert float((flat[:, :16] == -1.0).float().mean()) >= 0.10 and float((flat[:, 16:] == 0.0).float().mean()) >= 0.10      # zero padding: mask -1, the rest 0


# ---- part 4: the option through the pipeline --------------------------------------------------------------------------------------------
LOW = (24, 16)


def _network():
    """A network on which the CPU fp32 path is itself an accurate reference (tests/test_recurrence_gpu.py: the last layer scaled to
    0.05), with an AO channel that stays inside (0, 1) on most pixels, so that inverting it shows."""
    from isosurfacesuperresolution_amd import models
    torch.manual_seed(11)
    net = models.createNetwork('EnhanceNet', 4, 101, [0, 1, 2, 3, 4], 6, OPT)
    with torch.no_grad():
        last = net.postblock[8]
        last.weight.mul_(0.05); last.bias.mul_(0.05)
        last.weight[5].mul_(4.0); last.bias[5] = 0.5
    return net


def test_inverted_ao_checkpoint_through_the_pipeline():
    """A checkpoint saved with ``aoInverted: True`` and ``initialImage: "unshaded"`` on the frame's default fused route (packed assembly
    -> dataflow trunk -> fused tail; no part of that route has a lower size limit, so the frame is 24 x 16 -> 96 x 64, where the
    ray-marched object still covers a third of the pixels), three frames, teacher-forced against the module path on the same G-buffers
    (``LoadedModel.inference`` -> ``clamp_prediction`` -> ``ScreenSpaceShading`` with ``inverse_ao = True`` on the CPU)."""
    from isosurfacesuperresolution_amd import models, ops, volumes as V
    from isosurfacesuperresolution_amd.inference import DirectRenderer, LoadedModel
    from isosurfacesuperresolution_amd.pipeline import SuperResolutionPipeline, default_shading
    from isosurfacesuperresolution_amd.utils import clamp_prediction
    net = _network()
    state = {k: v.clone() for k, v in net.state_dict().items()}
    cnet = models.createNetwork('EnhanceNet', 4, 101, [0, 1, 2, 3, 4], 6, OPT)
    cnet.load_state_dict(state)
    params = lambda inv: {"aoInverted": inv, "initialImage": "unshaded"}
    renderer = DirectRenderer()
    renderer.load_dense(V.ejecta(64))
    cams = [V.orbit_camera(k) for k in range(3)]
    first_camera = V.quantize3(V.orbit_camera(-1))

    def pipeline(inv, graph=False):
        lm = LoadedModel.from_model(net, "cuda", parameters=params(inv))
        pipe = SuperResolutionPipeline(renderer, lm, default_shading("cuda", 30.0), LOW, graph=graph)
        pipe.set_static(fov=30.0, isovalue=0.34)
        return pipe

    def forced(pipe, previous_of):
        """Three frames; frame k's "previous" is ``previous_of[k - 1]`` where given."""
        pipe.reset()
        renderer.set_last_camera(first_camera)
        out = []
        for k, cam in enumerate(cams):
            if previous_of is not None and k > 0:
                pipe.previous = previous_of[k - 1].to(device="cuda", dtype=torch.float32).contiguous()
            rgb, raw = pipe.frame(cam)
            torch.cuda.synchronize()
            out.append((rgb.cpu().clone(), raw.cpu().clone(), pipe.gbuffer.cpu().clone()))
        return out

    pipe = pipeline(True)
    assert pipe.model.inverse_ao is True and pipe.model.initial_image_mode == "unshaded"
    free = forced(pipe, None)                                   # (its G-buffers are the sequence's; also the warm-up)
    gbufs = [g for _, _, g in free]
    assert all(int((g[..., 3] == 1).sum()) > 100 for g in gbufs)
    # the module path on the same G-buffers
    cm = LoadedModel.from_model(cnet.eval(), "cpu", parameters=params(True))
    shade = default_shading("cpu", 30.0)
    shade.inverse_ao = True
    module, prev = [], None
    for g in gbufs:
        raw = clamp_prediction(cm.inference(C.low_of(g), prev))
        module.append((shade(raw), raw))
        prev = raw
    ops.profile_enable(True)
    try:
        got = forced(pipe, [raw for _, raw in module])
        names = {n for n, _, _ in ops.profile_records()}
    finally:
        ops.profile_enable(False)
    assert "trunk_dataflow_kernel" in names and "conv3x3_split_tail_kernel" in names, names      # the default fused route
    for k, ((rgb, raw, g), (rgb_m, raw_m)) in enumerate(zip(got, module)):
        assert torch.equal(g, gbufs[k])
        e_raw, e_rgb = (raw - raw_m).abs().max().item(), (rgb - rgb_m).abs().max().item()
        print("frame %d: pipeline vs module path: raw %.2e rgb %.2e" % (k, e_raw, e_rgb))
        assert e_raw <= 1e-4 and e_rgb <= 1e-4, (k, e_raw, e_rgb)
    ao = module[1][1][:, 5]
    assert 0.2 <= float(((ao > 0.05) & (ao < 0.95)).float().mean())                    # the AO channel is not sitting on its clamps
    # 1. the same model saved without the option: a different image
    plain = forced(pipeline(False), [raw for _, raw in module])
    assert max((a[0] - b[0]).abs().max().item() for a, b in zip(got, plain)) > 1e-2
    assert (free[0][1][:, 5] - forced(pipeline(False), None)[0][1][:, 5]).abs().max().item() > 0      # (and the first frame's initial AO reaches the network)
    # 2. graph mode with the option set equals eager mode bit for bit (the flag is part of the capture's signature)
    def run(p):
        p.reset()
        renderer.set_last_camera(first_camera)
        out = []
        for k in range(5):
            rgb, raw = p.frame(V.orbit_camera(k), V.orbit_camera(k + 1))
            torch.cuda.synchronize()
            out.append((rgb.clone(), raw.clone()))
        return out
    eager, graphed = pipeline(True), pipeline(True, graph=True)
    assert graphed.graph and not eager.graph
    ref, rep = run(eager), run(graphed)
    assert graphed.graph_replays >= 1
    for k, ((rgb_a, raw_a), (rgb_b, raw_b)) in enumerate(zip(ref, rep)):
        assert torch.equal(raw_a, raw_b) and torch.equal(rgb_a, rgb_b), k
    sig = graphed._graph_signature()
    graphed.model.inverse_ao = False
    assert graphed._graph_signature() != sig                                           # a change of the flag drops the captured frames
    graphed.model.inverse_ao = True
