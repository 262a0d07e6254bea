"""GPU tests of the clip generator: ``clip_pack_kernel`` and ``clip_coverage_kernel`` (csrc/sr_dataset.hip) against their torch definitions
bit for bit, and ``datagen.generate_clips`` end to end -- every stored frame against per-frame renders, the direction of the flow, the
saved folder against the adopted buffers, one batch and one training step from them, and the launch and download counts."""
import argparse

import numpy as np
import pytest
import torch

import datagen_common as G
import device_dataset_common as C
import render_scenes
from train_route_common import observed

pytestmark = pytest.mark.gpu

PACK, COVERAGE = "clip_pack_kernel", "clip_coverage_kernel"
FRAMES, LOW, UPSCALE, AO = 3, 16, 4, 4
# scene A's spheres cover some thirty of the 16 x 16 low-resolution pixels: with this isovalue range and seed both clips, in both semantics,
# have 4 x 4 crops that are half covered in their first and last frame (none has such an 8 x 8 crop)
ISO, SEED, CROP = (0.1, 0.3), 1, 4
OPT = argparse.Namespace(upsample='bilinear', reconType='residual', useBN=False, numResidualLayers=2,
                         losses="l1:mask:1,l1:ao:1,l1:normal:10,l1:depth:10,temp-l2:color:0.1",
                         lossAO=0.0, lossAmbient=0.1, lossDiffuse=0.9, lossSpecular=0.0)


def _packed(h, w, r, offsets, sizes, device, seed=3):
    """Buffers of ``sizes`` filled with 7 after one ``pack_clip_frame`` of synthetic G-buffers at ``offsets``, and the kernel names."""
    from isosurfacesuperresolution_amd import ops
    operands = [t.to(device) for t in G.synthetic_gbuffers(seed, h, w, r)]
    bufs = [torch.full((n,), 7.0, device=device) for n in sizes]
    if device == "cpu":
        ops.pack_clip_frame(*operands, *bufs, offsets)
        return bufs, None
    assert ops.pack_clip_frame_supported(*operands)
    _, _, names = observed(lambda: ops.pack_clip_frame(*operands, *bufs, offsets))
    return bufs, names


# the float form (5 x 7: a width that is no multiple of four), the aligned form with one partly filled wave (8 x 12), with a ragged last
# wave (33 x 36 = 1188 pixels = 18 waves and 36 pixels) and with several workgroups of the low image (40 x 72).  Offsets: frame 0 of
# clip 0; a later frame of a second clip behind a 4 x 4 one (every start a multiple of four: the aligned form away from 0); and the last
# frame of a second clip whose high start was ROUNDED UP -- a 3 x 3 first clip at upscale 1 ends at 162 elements of high, the second
# starts at 164, and its low and flow starts (135, 54) are odd or even as they fall
@pytest.mark.parametrize("h,w", [(5, 7), (8, 12), (33, 36), (40, 72)])
@pytest.mark.parametrize("where", ["frame 0 of clip 0", "frame 1 of an aligned second clip", "last frame of a second clip with a rounded start"])
def test_pack_kernel_equals_the_definition(h, w, where):
    from isosurfacesuperresolution_amd import datagen
    T, n = 3, h * w
    r = 1 if "rounded" in where else UPSCALE
    frame = (6 * r * r * n, 5 * n, 2 * n)
    if where == "frame 0 of clip 0":
        offsets = (0, 0, 0)
    else:
        first = (3, 3) if "rounded" in where else (4, 4)
        rows, _ = datagen._clip_rows([first, (h, w)], T, r)
        assert (rows[1][0] != T * 6 * r * r * first[0] * first[1]) == ("rounded" in where) and rows[1][0] % 4 == 0
        j = T - 1 if "rounded" in where else 1
        offsets = tuple(s + j * f for s, f in zip(rows[1][:3], frame))
    sizes = tuple(o + f + 5 for o, f in zip(offsets, frame))
    want, _ = _packed(h, w, r, offsets, sizes, "cpu")
    got, names = _packed(h, w, r, offsets, sizes, "cuda")
    assert names == [PACK]                               # exactly one profile record per call
    for g, w_ in zip(got, want):
        assert G.same_bits_with_nans(g, w_)              # (a NaN alpha stays a NaN; everything else, negative zeros included, by its bits)
    assert C.negative_zeros(want[0]) > 0 and torch.isnan(want[1]).any()
    # without the NaN cases: torch.equal itself
    operands = G.synthetic_gbuffers(4, h, w, r, nan=False)
    from isosurfacesuperresolution_amd import ops
    bufs = {dev: [torch.zeros(s, device=dev) for s in sizes] for dev in ("cpu", "cuda")}
    for dev in bufs:
        ops.pack_clip_frame(*[t.to(dev) for t in operands], *bufs[dev], offsets)
    for g, w_ in zip(bufs["cuda"], bufs["cpu"]):
        assert torch.equal(g.cpu(), w_) and C.same_bits(g, w_)


def test_pack_kernel_with_unaligned_destinations_takes_the_float_form():
    """An aligned width behind odd offsets: 16-byte stores are impossible, the values are the same."""
    h, w, r = 8, 12, 4
    n = h * w
    offsets = (3, 1, 2)
    sizes = (offsets[0] + 6 * r * r * n + 1, offsets[1] + 5 * n + 1, offsets[2] + 2 * n + 1)
    want, _ = _packed(h, w, r, offsets, sizes, "cpu")
    got, names = _packed(h, w, r, offsets, sizes, "cuda")
    assert names == [PACK] and all(G.same_bits_with_nans(g, w_) for g, w_ in zip(got, want))


def test_pack_kernel_behind_two_to_the_31_elements():
    """The reference's dataset makes the flat high-resolution buffer longer than 2^31 elements: a frame packed behind that mark (the
    buffer is ``torch.empty``) equals the frame packed at offset 0 on the CPU."""
    from isosurfacesuperresolution_amd import ops
    free, _ = torch.cuda.mem_get_info()
    if free < 12 * 2 ** 30:
        pytest.skip("less than 12 GB of device memory free")
    h, w, r = 8, 12, 4
    n = h * w
    sizes = (6 * r * r * n, 5 * n, 2 * n)
    want, _ = _packed(h, w, r, (0, 0, 0), sizes, "cpu")
    offsets = (2 ** 31 + 4096, 2 ** 20 + 4, 2 ** 20 + 8)
    bufs = [torch.empty(o + s, dtype=torch.float32, device="cuda") for o, s in zip(offsets, sizes)]
    operands = [t.cuda() for t in G.synthetic_gbuffers(3, h, w, r)]
    _, _, names = observed(lambda: ops.pack_clip_frame(*operands, *bufs, offsets))
    assert names == [PACK]
    for buf, off, w_ in zip(bufs, offsets, want):
        assert G.same_bits_with_nans(buf[off:], w_)


def test_pack_without_the_entry_point_runs_the_definition_after_a_warning(monkeypatch):
    from isosurfacesuperresolution_amd import ops
    h, w, r = 8, 12, 2
    sizes = (6 * r * r * h * w, 5 * h * w, 2 * h * w)
    want, _ = _packed(h, w, r, (0, 0, 0), sizes, "cpu")
    monkeypatch.setattr(ops, "pack_clip_frame_supported", lambda *a: False)
    monkeypatch.setattr(ops, "_warned", set())
    operands = [t.cuda() for t in G.synthetic_gbuffers(3, h, w, r)]
    bufs = [torch.zeros(s, device="cuda") for s in sizes]
    with pytest.warns(RuntimeWarning, match="pack_clip_frame"):
        _, _, names = observed(lambda: ops.pack_clip_frame(*operands, *bufs, (0, 0, 0)))
    assert names == [] and all(G.same_bits_with_nans(g, w_) for g, w_ in zip(bufs, want))


@pytest.mark.parametrize("sizes", [((1, 1), (33, 37)), ((128, 128), (33, 37)), ((128, 128), (128, 128))])
def test_coverage_kernel_equals_the_definition(sizes):
    """Two clips (of different sizes, or of one size: then the result is a [clips, 2, H + 1, W + 1] tensor) behind an odd offset."""
    from isosurfacesuperresolution_amd import ops
    rng = np.random.default_rng(8)
    T, parts, rows, off = 3, [np.zeros(3, np.float32)], [], 3
    for H, W in sizes:
        low = rng.standard_normal((T, 5, H, W)).astype(np.float32)
        low[:, 0:3][rng.random((T, 3, H, W)) < 0.3] = 0.0
        low[:, 0][rng.random((T, H, W)) < 0.01] = np.nan
        rows.append((0, off, 0, H, W))
        parts.append(low.reshape(-1))
        off += low.size
    buf = torch.from_numpy(np.concatenate(parts))
    table = torch.tensor(rows)
    want = ops.clip_coverage(buf, table, T)
    got, _, names = observed(lambda: ops.clip_coverage(buf.cuda(), table.cuda(), T, rows=rows))
    assert names == [COVERAGE]
    assert got.dtype == torch.int32 and got.shape == want.shape and torch.equal(got.cpu(), want)
    assert want.dim() == (4 if sizes[0] == sizes[1] else 1) and int(want.max()) > 0
    again = ops.clip_coverage(buf.cuda(), table.cuda(), T)           # (the table read back instead of a host copy)
    assert torch.equal(again, got)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
class _Downloads:
    """Counts device-to-host copies: ``Tensor.cpu`` / ``numpy`` / ``tolist`` / ``item`` of a device tensor while active."""

    def __init__(self, monkeypatch):
        self.count = 0
        for name in ("cpu", "numpy", "tolist", "item"):
            real = getattr(torch.Tensor, name)

            def counted(t, *a, _real=real, **k):
                self.count += bool(t.is_cuda)
                return _real(t, *a, **k)
            monkeypatch.setattr(torch.Tensor, name, counted)


@pytest.fixture(scope="module")
def renderer():
    from isosurfacesuperresolution_amd import inference
    r = inference.DirectRenderer()
    r.load_dense(render_scenes.scene_a()[0])
    yield r
    for command, value in G.RENDERER_DEFAULTS:           # the library's state is the process's: leave it as a fresh one has it
        assert r.send_command(command, value) == 0
    r.set_last_camera((0, 0, -1), (0, 0, 0))


@pytest.fixture(scope="module", params=["gvdb", "cpu"])
def generated(request, renderer):
    from isosurfacesuperresolution_amd import datagen
    clips = datagen.generate_clips(renderer, 2, frames=FRAMES, high_res=LOW * UPSCALE, downscale=UPSCALE, ao_samples=AO, ao_radius=0.2,
                                   iso_range=ISO, seed=SEED, semantics=request.param)
    return request.param, clips


def _render(renderer, commands, shape):
    from isosurfacesuperresolution_amd import datagen
    datagen._send(renderer, commands)
    g = torch.empty(shape + (12,), dtype=torch.float32, device="cuda")
    assert renderer.render_direct(g) >= 0
    return g


def test_every_stored_frame_equals_the_definition_on_per_frame_renders(generated, renderer):
    from isosurfacesuperresolution_amd import datagen, ops
    semantics, clips = generated
    assert len(clips) == 2 and clips.rows[1][0] % 4 == 0 and all(t.is_cuda for t in (clips.high, clips.low, clips.flow))
    n, high_res = LOW * LOW, LOW * UPSCALE
    reversed_flow_differs = 0
    for k, params in enumerate(clips.parameters):
        if k == 0:                                                                    # the parameters are the seed's
            first = datagen.random_clip_parameters(np.random.RandomState(SEED), *ISO)
            assert np.array_equal(params.origin_start, first.origin_start) and params[5:10] == first[5:10]
        datagen._send(renderer, datagen.clip_commands(params, 0.2, semantics))
        cameras = datagen.clip_cameras(params, FRAMES)
        stored = clips.clip(k)
        for j, (origin, lookat, next_origin, next_lookat) in enumerate(cameras):
            renderer.set_last_camera(next_origin, next_lookat)
            low_g = _render(renderer, datagen.frame_commands(origin, lookat, (LOW, LOW), 0), (LOW, LOW))
            renderer.set_last_camera(next_origin, next_lookat)
            high_g = _render(renderer, datagen.frame_commands(origin, lookat, (high_res, high_res), AO), (high_res, high_res))
            flow = ops.fill_flow_gbuffer(low_g)
            want = [torch.zeros(s) for s in (6 * UPSCALE * UPSCALE * n, 5 * n, 2 * n)]
            ops._pack_clip_frame_torch(low_g.cpu(), high_g.cpu(), flow.cpu(), *want, (0, 0, 0))
            for got, w_ in zip(stored, want):
                assert torch.equal(got[j].cpu().reshape(-1), w_) and C.same_bits(got[j].reshape(-1), w_)
            assert (stored[1][j, 0] > 0).any() and (stored[1][j, 0] < 0).any()      # the surface is in view, and so is the background
            assert (stored[0][j, 5] != 0).any()                                       # the high frame carries ambient occlusion
            # the direction is the generator's: measured against the PREVIOUS camera (render_clip's) the flow is another one
            if j > 0:
                renderer.set_last_camera(cameras[j - 1][0], cameras[j - 1][1])
                back = _render(renderer, datagen.frame_commands(origin, lookat, (LOW, LOW), 0), (LOW, LOW))
                hit = back[..., 3] != 0
                assert torch.equal(back[..., 3:8], low_g[..., 3:8])
                reversed_flow_differs += int(not torch.equal(back[..., 8:10][hit], low_g[..., 8:10][hit]))
    assert reversed_flow_differs == 2 * (FRAMES - 1)


def test_the_saved_folder_and_the_adopted_buffers_give_the_same_clips_batch_and_step(generated, tmp_path):
    from isosurfacesuperresolution_amd import dataset_video as D, losses, models, train
    _, clips = generated
    crop = CROP
    clips.save(str(tmp_path))
    samples = clips.collect_samples(6, seed=3, crop=crop)          # (raises where no crop could be accepted: the host loop would not end)
    dd = D.collect_samples(str(tmp_path), 6, seed=3, crop=crop)
    assert samples == dd.samples
    uploaded, adopted = D.DeviceClips(dd, "cuda"), clips.device_clips(samples)
    for name in ("high", "low", "flow"):
        assert C.same_bits(getattr(adopted, name), getattr(uploaded, name))
        assert getattr(adopted, name).data_ptr() == getattr(clips, name).data_ptr()
    assert torch.equal(adopted.table, uploaded.table) and torch.equal(adopted.samples, uploaded.samples)
    host = next(iter(torch.utils.data.DataLoader(D.DatasetFromSamples(dd, False, 0.0), batch_size=2, shuffle=False)))
    batch = next(iter(D.DeviceBatchLoader(adopted, 2, test=False, test_fraction=0.0)))
    assert all(t.is_cuda for t in batch) and all(C.same_bits(g, w) for g, w in zip(batch, host))
    torch.manual_seed(124)
    net = models.createNetwork('EnhanceNet', 4, 101, [0, 1, 2, 3, 4], 6, OPT).cuda()
    crit = losses.LossNetUnshaded('cuda', 5, 6, 4 * crop, 2, OPT).cuda()
    optim, _ = train.make_optimizer(net)
    loss = train.train_step(net, crit, optim, batch, initial_image="zero")
    assert np.isfinite(loss) and all(torch.isfinite(q).all() for q in net.parameters())


def test_launch_and_download_counts(renderer, monkeypatch):
    """One clip of three frames: three pack launches while it is generated and nothing downloaded; the coverage tables are one more
    launch and the first download."""
    from isosurfacesuperresolution_amd import datagen
    downloads = _Downloads(monkeypatch)
    clips, _, names = observed(lambda: datagen.generate_clips(renderer, 1, frames=FRAMES, high_res=LOW * UPSCALE, downscale=UPSCALE,
                                                              ao_samples=AO, ao_radius=0.2, iso_range=ISO, seed=SEED, semantics="cpu"))
    assert [n for n in names if n in (PACK, COVERAGE)] == [PACK] * FRAMES
    assert downloads.count == 0
    tables, _, names = observed(clips.coverage_tables)
    assert [n for n in names if n in (PACK, COVERAGE)] == [COVERAGE]
    assert downloads.count >= 1 and tables[0].shape == (2, LOW + 1, LOW + 1) and tables[0].dtype == np.int32
    before = downloads.count
    clips.collect_samples(4, seed=1, crop=CROP)          # sampling works on the downloaded tables alone
    assert downloads.count == before


def test_command_line_writes_folders_that_the_dataset_reader_finds(renderer, tmp_path):
    """(Last in this file: the tool loads its own volume into the process's renderer.)  Scene A as a .vbx file behind a descriptor of two
    lines: one sub-folder of triples per volume, in the reference's shapes, and the list file ``_clip_paths`` understands."""
    from isosurfacesuperresolution_amd import datagen, dataset_video as D, vbx
    volumes = tmp_path / "volumes"
    volumes.mkdir()
    vbx.write_vbx(str(volumes / "scene-a.vbx"), render_scenes.scene_a()[0])
    (tmp_path / "inputs.dat").write_text("name min_iso max_iso\nscene-a.vbx 0.1 0.3\n")
    out = tmp_path / "out"
    datagen.main(["--descriptor", str(tmp_path / "inputs.dat"), "--volumes", str(volumes), "--out", str(out), "--clips", "2", "--frames", "3",
                  "--high", "64", "--downscale", "4", "--aosamples", "4", "--aoradius", "0.2", "--seed", str(SEED), "--semantics", "cpu"])
    assert (out / "clips.txt").read_text() == "scene-a\n"
    paths = D._clip_paths(str(out / "clips.txt"))
    assert len(paths) == 2
    clips = []
    for names in paths:
        high, low, flow = (np.load(n) for n in names)
        assert (high.shape, low.shape, flow.shape) == ((3, 6, 64, 64), (3, 5, 16, 16), (3, 2, 16, 16))
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in (high, low, flow))
        assert set(np.unique(low[:, 0])) == {-1.0, 1.0}                     # the surface and the background, as a mask in [-1, 1]
        clips.append((high, low, flow))
    samples = datagen.GeneratedClips.from_arrays(clips).collect_samples(3, seed=0, crop=CROP)
    assert len(samples) == 3
