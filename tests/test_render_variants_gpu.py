"""The ray-marcher's paths that share device code but are selected at run time: the AO instantiation of every kernel
variant, cost-ordered dispatch, the stats kernel and the capped-wave count of variant 2.  All of them must write the
frame variant 0 writes, bit for bit (test_render_gpu.py holds variants 0 and 4 to the oracle, AO channel included)."""
import ctypes
import time

import numpy as np
import pytest

from isosurfacesuperresolution_amd import volumes as V

pytestmark = pytest.mark.gpu

W, H = 72, 40                       # 9 x 5 tiles; the viewport of the AO test cuts through tiles on all four sides
TILES = 45


@pytest.fixture(scope="module")
def renderer():
    import torch
    assert torch.cuda.is_available()
    from isosurfacesuperresolution_amd.inference import DirectRenderer
    r = DirectRenderer()
    r.lib.isoDebugSetStatsBuffer.argtypes = [ctypes.c_ulonglong]
    return r


def _restore(r):
    r.set_kernel_variant(0)
    r.set_tile_order_mode(0)
    r.set_wave_cap(0)
    r.lib.isoDebugSetStatsBuffer(ctypes.c_ulonglong(0))
    r.send_command("aosamples", "0")


def _setup(r, fov, iso, ao_samples=0, ao_radius=0.05):
    for c, v in (("cameraLookAt", "0,0,0"), ("cameraUp", "0,1,0"), ("cameraFoV", "%.3f" % fov), ("isovalue", "%5.3f" % iso),
                 ("aoradius", "%5.3f" % ao_radius), ("aosamples", "%d" % ao_samples)):
        assert r.send_command(c, v) == 0


def _frame(r, w, h, k, viewport=None):
    import torch
    assert r.send_command("cameraOrigin", V.fmt3(V.orbit_camera(k))) == 0
    assert r.send_command("resolution", "%d,%d" % (w, h)) == 0
    assert r.send_command("viewport", "%d,%d,%d,%d" % tuple(viewport or (0, 0, w, h))) == 0
    out = torch.full((h, w, 12), 7.0, dtype=torch.float32, device="cuda")
    r.render_async(out, torch.cuda.current_stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _sequence(r, frames, viewport=None):
    """frames: (w, h, k).  The flow reference of the first frame is pinned, so that two sequences can be compared."""
    r.set_last_camera(V.quantize3(V.orbit_camera(frames[-1][2])))
    return [_frame(r, w, h, k, viewport) for (w, h, k) in frames]


def test_ao_instantiation_of_every_variant_writes_variant_0s_frame(renderer):
    vp = (5, 3, 61, 37)
    frames = [(W, H, 3), (W, H, 40), (W, H, 11)]
    try:
        renderer.load_dense(V.ejecta(64))
        _setup(renderer, 30.0, 0.34, ao_samples=4, ao_radius=0.05)
        renderer.set_kernel_variant(0)
        ref = _sequence(renderer, frames, vp)
        inside = np.zeros((H, W), dtype=bool)
        inside[vp[1]:vp[3], vp[0]:vp[2]] = True
        blank = np.zeros(12, dtype=np.float32)
        blank[10] = 1.0
        for img in ref:
            assert img[..., 3].sum() > 50 and (img[..., 10][img[..., 3] == 1] < 1.0).any()      # hits, and occluded ones
            assert np.array_equal(img[~inside], np.broadcast_to(blank, img[~inside].shape))
        for variant in (1, 2, 3, 4, 5):
            renderer.set_kernel_variant(variant)
            got = _sequence(renderer, frames, vp)
            for f, (a, b) in enumerate(zip(got, ref)):
                assert np.array_equal(a, b), "variant %d, frame %d: %d values differ" % (variant, f, int((a != b).sum()))
    finally:
        _restore(renderer)


def test_cost_ordered_dispatch_writes_the_same_frames(renderer):
    """The first frame at a resolution runs unordered and measures, the second runs in the order built from the first.
    360 x 256 is 1440 tiles: more than four per CU (mode 2's lightest-first part runs), fewer than ISO_ORDER_MAX_TILES;
    the last frame finds an order stored for another resolution.  Only the frames are compared: the library has no getter that
    says the ordered path ran, so an order that silently never engaged would pass here too."""
    frames = [(W, H, 3), (W, H, 5), (360, 256, 7), (360, 256, 9), (W, H, 11)]
    try:
        renderer.load_dense(V.sphere64())
        _setup(renderer, 45.0, 0.5)
        renderer.set_kernel_variant(0)
        assert renderer.set_tile_order_mode(3) == -1
        assert renderer.set_tile_order_mode(0) == 0
        ref = _sequence(renderer, frames)
        assert all(img[..., 3].sum() > 50 for img in ref)
        for mode in (1, 2):
            assert renderer.set_tile_order_mode(mode) == 0
            got = _sequence(renderer, frames)
            for f, (a, b) in enumerate(zip(got, ref)):
                assert np.array_equal(a, b), "mode %d, frame %d: %d values differ" % (mode, f, int((a != b).sum()))
    finally:
        _restore(renderer)


def test_stats_kernel_is_the_render_plus_counters(renderer):
    import torch
    try:
        renderer.load_dense(V.ejecta(64))
        _setup(renderer, 30.0, 0.34)
        counters = {}
        for variant in (0, 4, 5):
            renderer.set_kernel_variant(variant)
            plain = _sequence(renderer, [(W, H, 3)])[0]
            stats = torch.zeros((TILES, 6), dtype=torch.int64, device="cuda")
            renderer.lib.isoDebugSetStatsBuffer(ctypes.c_ulonglong(stats.data_ptr()))
            img = _sequence(renderer, [(W, H, 3)])[0]
            renderer.lib.isoDebugSetStatsBuffer(ctypes.c_ulonglong(0))
            assert np.array_equal(img, plain), "variant %d: the stats kernel renders another frame" % variant
            s = stats.cpu().numpy()
            mask = np.zeros((40, 72), dtype=np.int64)
            mask[:H, :W] = img[..., 3] == 1
            hits = mask.reshape(5, 8, 9, 8).sum(axis=(1, 3)).reshape(TILES)          # raster tile t = ty * 9 + tx
            assert hits.sum() > 50
            assert np.array_equal(s[:, 5], hits)
            assert (s[:, 1] <= s[:, 4]).all()
            assert (s[:, 0] > 0).all()
            counters[variant] = s[:, 1:6]
        # the three traversals take the same samples and visit the same leaves, ray by ray
        assert np.array_equal(counters[4], counters[0]) and np.array_equal(counters[5], counters[0])
    finally:
        _restore(renderer)


@pytest.mark.parametrize("cap", [0, 8, 1024])
def test_residency_target_agrees_with_the_launcher(renderer, cap):
    """isoGateResident waits for as many waves as the renders said they launched: were the two counts to differ, the gate
    would sit out its timeout (bound on the elapsed time as in test_residency_gate_returns)."""
    import torch
    try:
        renderer.load_dense(V.ejecta(64))
        _setup(renderer, 30.0, 0.34)
        renderer.set_kernel_variant(0)
        ref = _sequence(renderer, [(W, H, 3)])[0]
        renderer.set_kernel_variant(2)
        assert renderer.set_wave_cap(cap) == 0
        img = _sequence(renderer, [(W, H, 3)])[0]
        s = torch.cuda.current_stream()
        t0 = time.perf_counter()
        assert renderer.gate_resident(s, 100000) == 0               # 0.1 s timeout must not be needed
        torch.cuda.synchronize()
        assert time.perf_counter() - t0 < 0.05
        assert ref[..., 3].sum() > 50
        assert np.array_equal(img, ref)
    finally:
        _restore(renderer)
