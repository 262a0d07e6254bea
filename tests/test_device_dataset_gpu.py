"""GPU tests of the device-resident training clips: ``clip_gather_kernel`` (csrc/sr_dataset.hip) against the CPU definition of
``ops.gather_clips`` bit for bit, its launch count, its index guard and its 64-bit addressing, and ``DeviceBatchLoader`` through
``train.fit`` with graphed steps."""
import argparse
import types

import numpy as np
import pytest
import torch

import device_dataset_common as C
from train_route_common import observed

pytestmark = pytest.mark.gpu

KERNEL = "clip_gather_kernel"
OPT = argparse.Namespace(upsample='bilinear', reconType='residual', useBN=False, numResidualLayers=10,
                         losses="l1:mask:1,l1:ao:1,l1:normal:10,l1:depth:10,temp-l2:color:0.1",
                         lossAO=0.0, lossAmbient=0.1, lossDiffuse=0.9, lossSpecular=0.0)


@pytest.fixture(scope="module")
def fixtures():
    """{low channels: (DatasetData, CPU clips, device clips, {augment: the CPU definition's batch})}, computed once."""
    from isosurfacesuperresolution_amd import dataset_video as D, ops
    out = {}
    for low_channels in (5, 8):
        dd = C.dataset(low_channels)
        cpu = D.DeviceClips(dd, "cpu")
        want = {aug: ops.gather_clips(cpu, cpu.samples, torch.tensor(C.BATCH), C.CROP, aug) for aug in (False, True)}
        out[low_channels] = (dd, cpu, D.DeviceClips(dd, "cuda"), want)
    return out


@pytest.mark.parametrize("low_channels", [5, 8])
@pytest.mark.parametrize("augment", [False, True])
def test_one_launch_equals_the_cpu_definition_and_repeats(fixtures, low_channels, augment):
    from isosurfacesuperresolution_amd import ops
    _, _, clips, want = fixtures[low_channels]
    idx = torch.tensor(C.BATCH, device="cuda")
    assert ops.gather_clips_supported(clips, clips.samples, idx, C.CROP)
    got, _, names = observed(lambda: ops.gather_clips(clips, clips.samples, idx, C.CROP, augment))
    assert names == [KERNEL]                        # exactly one launch per batch
    assert all(t.is_cuda for t in got)
    for g, w in zip(got, want[augment]):
        assert C.same_bits(g, w)
    again = ops.gather_clips(clips, clips.samples, idx, C.CROP, augment)
    assert all(C.same_bits(a, g) for a, g in zip(again, got))


@pytest.mark.parametrize("augment", [False, True])
def test_the_workloads_crop_on_a_width_that_is_no_multiple_of_sixteen_floats(augment):
    """c = 32 (128 x 128 high-resolution crops) on one 40 x 52 clip: several workgroups per sample and a stride loop."""
    from isosurfacesuperresolution_amd import dataset_video as D, ops
    rng = np.random.default_rng(4)
    high, low, flow = C.random_clip(rng, 3, 8, 6, 40, 52, 4)
    samples = [C.make_sample(D, 0, x0, y0, 32, 4, mode) for x0, y0 in ((0, 0), (8, 20), (3, 5)) for mode in range(4)]
    dd = D.DatasetData(samples, [high], [low], [flow], 8, 6, 32, 3)
    cpu, dev = D.DeviceClips(dd, "cpu"), D.DeviceClips(dd, "cuda")
    order = [7, 0, 11, 4, 9, 2, 5, 10, 1]
    want = ops.gather_clips(cpu, cpu.samples, torch.tensor(order), 32, augment)
    got, _, names = observed(lambda: ops.gather_clips(dev, dev.samples, torch.tensor(order, device="cuda"), 32, augment))
    assert names == [KERNEL]
    assert got[2].shape == (9, 3, 6, 128, 128)
    for g, w in zip(got, want):
        assert C.same_bits(g, w)


@pytest.mark.parametrize("case", ["upscale 2", "odd high offset"])
def test_the_float_by_float_form_of_the_high_resolution_part(case):
    """16 bytes per lane need r to be a multiple of four and clips on multiples of four elements; everything else takes the other
    instantiation of the kernel, one float per item: r = 2, and r = 4 with the clip at an odd element offset."""
    from isosurfacesuperresolution_amd import dataset_video as D, ops
    rng = np.random.default_rng(6)
    r = 2 if case == "upscale 2" else 4
    H, W = 12, 19
    high, low, flow = C.random_clip(rng, C.T, 8, 6, H, W, r)
    samples = [C.make_sample(D, 0, x0, y0, 8, r, mode) for x0, y0 in ((0, 0), (4, 11), (1, 3)) for mode in range(4)]
    cpu = D.DeviceClips(D.DatasetData(samples, [high], [low], [flow], 8, 6, 8, C.T), "cpu")
    assert cpu.upscale == r
    idx = torch.tensor([11, 3, 6, 0, 9, 5])
    want = ops.gather_clips(cpu, cpu.samples, idx, 8, True)
    dev = D.DeviceClips(D.DatasetData(samples, [high], [low], [flow], 8, 6, 8, C.T), "cuda")
    if case == "odd high offset":
        shifted = torch.empty(dev.high.numel() + 1, dtype=torch.float32, device="cuda")
        shifted[1:].copy_(dev.high)
        table = dev.table.clone()
        table[0, 0] = 1
        dev = types.SimpleNamespace(high=shifted, low=dev.low, flow=dev.flow, table=table, frames=C.T, low_channels=8, high_channels=6,
                                    upscale=r, high_quad_aligned=False)
    got, _, names = observed(lambda: ops.gather_clips(dev, cpu.samples.cuda(), idx.cuda(), 8, True))
    assert names == [KERNEL]
    for g, w in zip(got, want):
        assert C.same_bits(g, w)


def test_a_library_without_the_entry_point_runs_the_definition_after_a_warning(fixtures, monkeypatch):
    from isosurfacesuperresolution_amd import ops
    _, _, clips, want = fixtures[8]
    monkeypatch.setattr(ops, "gather_clips_supported", lambda *a: False)
    monkeypatch.setattr(ops, "_warned", set())
    with pytest.warns(RuntimeWarning, match="gather_clips"):
        got, _, names = observed(lambda: ops.gather_clips(clips, clips.samples, torch.tensor(C.BATCH, device="cuda"), C.CROP, True))
    assert names == [] and all(t.is_cuda for t in got)
    for g, w in zip(got, want[True]):
        assert C.same_bits(g, w)


def test_an_index_outside_the_sample_table_is_clamped(fixtures):
    from isosurfacesuperresolution_amd import ops
    _, _, clips, _ = fixtures[8]
    n = clips.num_samples
    got = ops.gather_clips(clips, clips.samples, torch.tensor([-1, n + 5, 3], device="cuda"), C.CROP, True)
    want = ops.gather_clips(clips, clips.samples, torch.tensor([0, n - 1, 3], device="cuda"), C.CROP, True)
    torch.cuda.synchronize()
    assert all(C.same_bits(g, w) for g, w in zip(got, want))


def test_a_clip_beyond_two_to_the_31_elements_of_the_flat_buffer():
    """The reference's dataset makes the flat high-resolution buffer longer than 2^31 elements: one small clip placed behind that
    mark (the buffer is ``torch.empty``, only the clip is written) comes back as the same clip at offset 0 does on the CPU."""
    from isosurfacesuperresolution_amd import dataset_video as D, ops
    free, _ = torch.cuda.mem_get_info()
    if free < 12 * 2 ** 30:
        pytest.skip("less than 12 GB of device memory free")
    rng = np.random.default_rng(9)
    H, W = 12, 20
    high, low, flow = C.random_clip(rng, C.T, 5, 6, H, W, 4)
    samples = [C.make_sample(D, 0, x0, y0, 8, 4, mode) for x0, y0 in ((0, 0), (4, 12), (1, 3)) for mode in range(4)]
    cpu = D.DeviceClips(D.DatasetData(samples, [high], [low], [flow], 5, 6, 8, C.T), "cpu")
    idx = torch.arange(12)
    want = ops.gather_clips(cpu, cpu.samples, idx, 8, True)
    offsets = (2 ** 31 + 4096, 2 ** 20 + 3, 2 ** 20 + 1)              # high beyond the mark; low and flow at odd element offsets
    buffers = []
    for off, a in zip(offsets, (high, low, flow)):
        buf = torch.empty(off + a.size, dtype=torch.float32, device="cuda")
        buf[off:].copy_(torch.from_numpy(a).reshape(-1))
        buffers.append(buf)
    clips = types.SimpleNamespace(high=buffers[0], low=buffers[1], flow=buffers[2], frames=C.T, low_channels=5, high_channels=6, upscale=4,
                                  high_quad_aligned=True, table=torch.tensor([offsets + (H, W)], dtype=torch.int64, device="cuda"))
    got, _, names = observed(lambda: ops.gather_clips(clips, cpu.samples.cuda(), idx.cuda(), 8, True))
    assert names == [KERNEL]
    for g, w in zip(got, want):
        assert C.same_bits(g, w)


def test_device_loader_through_the_fit_driver_with_graphed_steps(tmp_path):
    """The clips and the network of test_fit_gpu.py's first test (V.cloud(512) through this package's ray-marcher, 4 clips of 5 frames,
    10 samples), two epochs of ``train.fit`` fed by ``DeviceBatchLoader``: the first batch is the host loader's bit for bit, the
    losses are finite and the checkpoint loads.  (No comparison of the trained weights with a host-fed run: the warp's backward adds
    with float atomics, two runs differ.)"""
    from isosurfacesuperresolution_amd import dataset_video as D, inference, losses, models, train, volumes as V
    from isosurfacesuperresolution_amd.dataset_video import render_clip
    r = inference.DirectRenderer()
    r.load_dense(V.cloud(512))
    clips = tmp_path / "clips"
    clips.mkdir()
    for c in range(4):
        origins = [V.orbit_camera(8 * c + k, K=64, distance=1.8, pitch=0.3) for k in range(5)]
        high, low, flow = render_clip(r, origins, (128, 72), isovalue=0.30, ao_samples=8, ao_radius=0.05)
        np.save(clips / ("high_%05d.npy" % c), high)
        np.save(clips / ("low_%05d.npy" % c), low)
        np.save(clips / ("flow_%05d.npy" % c), flow)
    dd = D.collect_samples(str(clips), 10, seed=4)
    resident = D.DeviceClips(dd, "cuda")
    train_loader = D.DeviceBatchLoader(resident, 4, test=False, test_fraction=0.2)
    test_loader = D.DeviceBatchLoader(resident, 2, test=True, test_fraction=0.2)
    assert (len(train_loader), len(test_loader)) == (2, 1)
    host_first = next(iter(torch.utils.data.DataLoader(D.DatasetFromSamples(dd, False, 0.2), batch_size=4, shuffle=False)))
    first = next(iter(train_loader))
    assert all(t.is_cuda for t in first) and all(C.same_bits(g, w) for g, w in zip(first, host_first))
    torch.manual_seed(124)
    net = models.createNetwork('EnhanceNet', 4, 101, [0, 1, 2, 3, 4], 6, OPT)
    crit = losses.LossNetUnshaded('cuda', 5, 6, 128, 16, OPT).cuda()
    net, hist = train.fit(net, crit, train_loader, test_loader, str(tmp_path / "run00000"), 2, dict(vars(OPT), initialImage="zero"),
                          device="cuda", lr=2e-4, lr_step=100, graphed=True, initial_image="zero", log=lambda *_: None)
    assert [h['epoch'] for h in hist] == [1, 2]
    assert all(np.isfinite(h['train_loss']) and np.isfinite(h['test']['total_loss']) for h in hist)
    lm = inference.LoadedModel(hist[-1]['checkpoint'], "cuda", 4)
    out = lm.inference(torch.rand(1, 12, 72, 128, device="cuda"), None)
    assert out.shape == (1, 6, 288, 512) and torch.isfinite(out).all()
