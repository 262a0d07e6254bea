"""Which kernel form a shape takes, pinned through the public profiling API.

Every form of one layer computes the same bits, so a parity test cannot see a launch that took another form than the dispatcher
meant it to: only the frame rate would.  Each case here is ONE launch on random data; the assertion is the kernel name the library
recorded for it (``ops.profile_records``) and the way the call returned.  Values are compared only where a case says so.

The thresholds restated here are the dispatchers' own (csrc/sr_conv_split.hip, csrc/sr_conv3x3.hip):
    split, plain layers   tiles = N ceil(W / 32) ceil(H / 8) ceil(Cout / 64),  tiles2 the same with 2-row tiles,  slots = 2 CUs
                          quads (W % 4 == 0, aligned input) and tiles < 256 and tiles2 >= 64    -> conv3x3_split_rows2_kernel
                          quads and tiles > 4 slots                                             -> conv3x3_split_stream_kernel
                          everything else                                                       -> conv3x3_split_kernel<false>
    split, upsampling     64 -> 64 channels                                                     -> conv3x3_split_ups3_kernel
                          anything else                                                         -> conv3x3_split_kernel<true>
    exact                 groups = ceil(Cout / 32),  big = N ceil(W / 32) ceil(H / 16) groups,  small = N ceil(W / 32) ceil(H / 4) groups
                          big < 384 and small <= 160 and no upsampling                          -> conv3x3_rowsplit_kernel
                          big < 384                                                             -> conv3x3_fwd2_kernel<., 1>
                          otherwise                                                             -> conv3x3_fwd2_kernel<., 4>
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

TILE = "conv3x3_split_kernel<false>"
TILE_UPS = "conv3x3_split_kernel<true>"
ROWS2 = "conv3x3_split_rows2_kernel"
STREAM = "conv3x3_split_stream_kernel"
UPS3 = "conv3x3_split_ups3_kernel"


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.rand(*shape, generator=g) * 2 - 1).cuda()


def _layer(cin, cout):
    g = torch.Generator().manual_seed(1000 * cin + cout)
    w = ((torch.rand(cout, cin, 3, 3, generator=g) * 2 - 1) / (3.0 * cin ** 0.5)).cuda()
    return w, (torch.rand(cout, generator=g) - 0.5).cuda()


def _recorded(fn):
    """(what ``fn`` returned, the kernel names recorded while it ran)"""
    from isosurfacesuperresolution_amd import ops
    torch.cuda.synchronize()
    ops.profile_enable(True)
    try:
        with torch.no_grad():
            out = fn()
        torch.cuda.synchronize()
        names = [r[0] for r in ops.profile_records()]
    finally:
        ops.profile_enable(False)
    return out, names


# (act, with a residual): each plain-layer case runs bare, with a fused skip, and with a ReLU
VARIANTS = [("none", False), ("none", True), ("relu", False)]


def _split_plain(n, h, w, act, with_res, cin=16, cout=32, seed=0):
    from isosurfacesuperresolution_amd import ops
    x = _rand(n, cin, h, w, seed=seed)
    wt, b = _layer(cin, cout)
    res = _rand(n, cout, h, w, seed=seed + 1) if with_res else None
    return _recorded(lambda: ops.conv3x3_split(x, wt, b, act=act, residual=res))


def _one_round_images():
    """N images of 64 x 256 (64 tiles each) that fill four rounds of the 2 CUs slots and not a tile more: tiles <= 4 slots < tiles + 64
    (tiles == 4 slots wherever the CU count is a multiple of 8: N = 32 on 256 CUs)."""
    return (4 * 2 * _cus()) // 64


@pytest.mark.parametrize("act,with_res", VARIANTS)
def test_split_small_batch_takes_the_two_row_form(act, with_res):
    y, names = _split_plain(4, 32, 32, act, with_res)           # tiles = 16, tiles2 = 64
    assert names == [ROWS2] and y.shape == (4, 32, 32, 32)


@pytest.mark.parametrize("act,with_res", VARIANTS)
def test_split_one_tile_short_of_the_two_row_form_takes_the_tile_form(act, with_res):
    y, names = _split_plain(1, 126, 32, act, with_res)          # tiles = 16, tiles2 = 63
    assert names == [TILE] and y.shape == (1, 32, 126, 32)


@pytest.mark.parametrize("act,with_res", VARIANTS)
def test_split_one_round_boundary(act, with_res):
    """Four rounds of the slots: the tile form; one image more: the persistent form.  The shared images come out bit-identical."""
    n = _one_round_images()
    assert n >= 1
    y0, names0 = _split_plain(n, 64, 256, act, with_res, seed=7)
    assert names0 == [TILE]
    # the same first n images, one more behind them
    from isosurfacesuperresolution_amd import ops
    x = torch.cat([_rand(n, 16, 64, 256, seed=7), _rand(1, 16, 64, 256, seed=99)])
    res = torch.cat([_rand(n, 32, 64, 256, seed=8), _rand(1, 32, 64, 256, seed=98)]) if with_res else None
    wt, b = _layer(16, 32)
    y1, names1 = _recorded(lambda: ops.conv3x3_split(x, wt, b, act=act, residual=res))
    assert names1 == [STREAM]
    assert torch.equal(y0, y1[:n])


@pytest.mark.parametrize("act,with_res", VARIANTS)
@pytest.mark.parametrize("size", ["small", "large"])
def test_split_rows_that_are_no_quads_take_the_tile_form_at_any_size(size, act, with_res):
    """W = 30: no 16-byte pixel groups, so neither the two-row nor the persistent form, whatever the tile count says."""
    n, h = (4, 32) if size == "small" else (_one_round_images() + 1, 512)        # small: tiles2 = 64; large: 64 tiles per image, past four rounds
    y, names = _split_plain(n, h, 30, act, with_res)
    assert names == [TILE] and y.shape == (n, 32, h, 30)


def test_split_upsampling_64_to_64_takes_the_three_per_cu_form():
    from isosurfacesuperresolution_amd import ops
    x = _rand(1, 64, 8, 16)
    wt, b = _layer(64, 64)
    y, names = _recorded(lambda: ops.conv3x3_split(x, wt, b, act="relu", upsample2x=True))
    assert names == [UPS3] and y.shape == (1, 64, 16, 32)


def test_split_upsampling_64_to_32_takes_the_tile_form():
    from isosurfacesuperresolution_amd import ops
    x = _rand(1, 64, 8, 16)
    wt, b = _layer(64, 32)
    y, names = _recorded(lambda: ops.conv3x3_split(x, wt, b, act="relu", upsample2x=True))
    assert names == [TILE_UPS] and y.shape == (1, 32, 16, 32)


def test_split_upsampling_with_a_skip_of_odd_plane_stride_falls_through_to_the_tile_form():
    """The three-per-CU form stores quads only: a residual whose planes are not a multiple of four floats apart sends the 64 -> 64
    layer to the tile form, and that is the name recorded."""
    from isosurfacesuperresolution_amd import ops
    x = _rand(1, 64, 8, 16)
    wt, b = _layer(64, 64)
    res = _rand(1, 64, 16, 32, seed=5)
    plane = 16 * 32 + 1
    odd = torch.empty(64 * plane, device="cuda").as_strided((1, 64, 16, 32), (64 * plane, plane, 32, 1))
    odd.copy_(res)
    y0, names0 = _recorded(lambda: ops.conv3x3_split(x, wt, b, act="relu", residual=res, upsample2x=True))
    y1, names1 = _recorded(lambda: ops.conv3x3_split(x, wt, b, act="relu", residual=odd, upsample2x=True))
    assert names0 == [UPS3]
    assert names1 == [TILE_UPS]
    assert torch.allclose(y0, y1, rtol=0.0, atol=1e-4)


def test_split_upsampling_of_unaligned_rows_is_refused_and_the_caller_falls_back():
    """Input width 6: the library answers -3 and records nothing; ``ops.conv3x3_split`` resizes first and runs a plain layer."""
    from isosurfacesuperresolution_amd import ops
    lib = ops._sr()
    x = _rand(1, 64, 8, 6)
    wt, b = _layer(64, 64)
    wq = ops._prepare_split(wt)
    y = torch.empty(1, 64, 16, 12, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc, names = _recorded(lambda: lib.isrConv3x3ForwardSplit(x.data_ptr(), wq.data_ptr(), b.data_ptr(), None, y.data_ptr(), 1, 64, 16, 12, 64, 1, 0.0, 1,
                                                             48, 64 * 48, 192, 64 * 192, 0, 0, stream))
    assert rc == -3 and names == []
    y1, names1 = _recorded(lambda: ops.conv3x3_split(x, wt, b, act="relu", upsample2x=True))
    assert names1 == [TILE] and y1.shape == (1, 64, 16, 12)
    y2, _ = _recorded(lambda: ops.conv3x3_split(ops.bilinear_upsample2x(x), wt, b, act="relu"))
    assert torch.equal(y1, y2)


def _packed_shapes():
    """(H, W, the form of the UNPACKED call) of one 16-channel image"""
    rounds = (4 * 2 * _cus()) // 32 + 1          # tile rows of a 1024-wide image (32 tiles each) that no longer fit four rounds
    return [(126, 32, TILE), (128, 32, ROWS2), (8 * rounds, 1024, STREAM)]


@pytest.mark.parametrize("shape", [0, 1, 2])
def test_packed_hand_over_always_takes_the_tile_form(shape):
    """The packed-split layouts are known to the tile form only: packed in, packed out or both run it on every shape, whatever form
    the same layer takes unpacked; and the next unpacked launch is routed as if nothing had happened."""
    from isosurfacesuperresolution_amd import ops
    h, w, form = _packed_shapes()[shape]
    x = _rand(1, 16, h, w, seed=shape)
    wt, b = _layer(16, 32)
    y, names = _recorded(lambda: ops.conv3x3_split(x, wt, b, act="relu"))
    assert names == [form]
    packed, names = _recorded(lambda: ops.conv3x3_split_packed(x, wt, b, act="relu"))
    assert names == [TILE]
    xp = ops.pack_split(x)
    y2, names = _recorded(lambda: ops.conv3x3_split_from_packed(xp, wt, b, act="relu"))
    assert names == [TILE]
    assert torch.equal(y, y2)
    packed2, names = _recorded(lambda: ops.conv3x3_split_from_packed(xp, wt, b, act="relu", packed_out=True))
    assert names == [TILE]
    assert torch.equal(packed.to_float(), packed2.to_float())
    # restore after override: the two-row shape still takes the two-row form
    _, names = _split_plain(4, 32, 32, "none", False)
    assert names == [ROWS2]
    _, names = _recorded(lambda: ops.conv3x3_split(x, wt, b, act="relu"))
    assert names == [form]


@pytest.fixture
def exact_mode():
    from isosurfacesuperresolution_amd import ops
    old = ops.SPLIT_F16
    ops.SPLIT_F16 = False
    yield
    ops.SPLIT_F16 = old


# Cout 64: two 32-channel groups.  (N, h, w of the input, upsample, expected) on either side of small <= 160 and of big < 384
EXACT = [
    (10, 32, 32, False, "conv3x3_rowsplit_kernel"),             # big = 40, small = 160
    (11, 32, 32, False, "conv3x3_fwd2_kernel<false,1>"),        # big = 44, small = 176
    (1, 3056, 32, False, "conv3x3_fwd2_kernel<false,1>"),       # big = 382
    (1, 3072, 32, False, "conv3x3_fwd2_kernel<false,4>"),       # big = 384
    (1, 16, 16, True, "conv3x3_fwd2_kernel<true,1>"),           # big = 4, small = 16: the row form has no upsampling variant
    (1, 1528, 16, True, "conv3x3_fwd2_kernel<true,1>"),         # big = 382
    (1, 1536, 16, True, "conv3x3_fwd2_kernel<true,4>"),         # big = 384
]


@pytest.mark.parametrize("n,h,w,ups,expected", EXACT)
def test_exact_forward_forms(n, h, w, ups, expected, exact_mode):
    from isosurfacesuperresolution_amd import ops
    x = _rand(n, 16, h, w)
    wt, b = _layer(16, 64)
    y, names = _recorded(lambda: ops.conv3x3(x, wt, b, act="relu", upsample2x=ups))
    assert names == [expected]
    assert y.shape == ((n, 64, 2 * h, 2 * w) if ups else (n, 64, h, w))


def test_a_refused_launch_takes_the_range_flag_with_it():
    """``isrSetRangeFlag`` arms the NEXT launch.  A launch that fails validation has taken the flag: the launch after it must not
    write the word."""
    from isosurfacesuperresolution_amd import ops
    lib = ops._sr()
    x = _rand(1, 16, 16, 32)
    wt, b = _layer(16, 32)
    wq = ops._prepare_split(wt)
    y = torch.empty(1, 32, 16, 32, device="cuda")
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch(h):
        return lib.isrConv3x3ForwardSplit(x.data_ptr(), wq.data_ptr(), b.data_ptr(), None, y.data_ptr(), 1, 16, h, 32, 32, 0, 0.0, 0,
                                          512, 16 * 512, 512, 32 * 512, 0, 0, stream)

    lib.isrSetRangeFlag(word.data_ptr())
    rc, names = _recorded(lambda: launch(0))
    assert rc == -1 and names == []
    rc, names = _recorded(lambda: launch(16))
    assert rc == 0 and names == [TILE]
    assert word.item() == 0
    # (the word is written when the launch that follows the arming is the valid one)
    lib.isrSetRangeFlag(word.data_ptr())
    assert launch(16) == 0
    torch.cuda.synchronize()
    assert word.item() != 0


def test_forced_persistent_form_and_back(diag_lib):
    """Diagnostics build: ``isrDebugSetSplitAlgo(3)`` forces the persistent form on a shape of one round; resetting it restores the tile form."""
    _, names = _split_plain(1, 126, 32, "none", False)
    assert names == [TILE]
    diag_lib.isrDebugSetSplitAlgo(3)
    try:
        _, names = _split_plain(1, 126, 32, "none", False)
    finally:
        diag_lib.isrDebugSetSplitAlgo(1)
    assert names == [STREAM]
    _, names = _split_plain(1, 126, 32, "none", False)
    assert names == [TILE]
