"""``ops.discriminator_input`` on the device (``isrDiscrInputForward`` / ``isrDiscrInputBackward``, csrc/sr_train.hip) against the module
composition in fp64 on the CPU (discr_input_common.composition).

Bars come from the reference, not from the kernel: four times the distance of the SAME composition in fp32 on the CPU from fp64;
values not below 1e-6, gradients relative to the largest |gradient| of the tensor, not below 1e-5.  Pixels planted exactly on kinks
(discr_input_common.plant) are measured and printed per kind, separately from the rest: the gradient of a normal of length 5e-8 is
1e7 times its upstream, which would make a bar relative to "the tensor's largest" say nothing about the other pixels.  Every channel
of every border pixel, values and gradients, is exactly 0; two runs give the same bits; a forward is ONE launch of this library and a
backward is one."""
import itertools
import warnings

import pytest
import torch

import gan_common as C
from discr_input_common import CHANNELS, CLEAR, COMBINATIONS, compare, composition, kink_clearance, make_shading, operands, pixel_sets
from isosurfacesuperresolution_amd import ops
from train_route_common import observed

pytestmark = pytest.mark.gpu

FWD, BWD = "discr_input_fwd_kernel", "discr_input_bwd_kernel"
SHAPES = [(2, 16, 16, 2), (3, 12, 20, 0), (1, 8, 8, 3)]                    # (N, H, W, pad): the fixture's, non-square borderless, 2 x 2 interior
FALLBACK_SHAPES = [(2, 10, 14, 1), (1, 8, 8, 4)]                           # a width that is no multiple of 4, a border that leaves nothing
# (order, cur_raw_normal, inverse_ao, ao_strength)
VARIANTS = list(itertools.product((0, 1), (0, 1), (False, True), (0.0, 0.5, 1.0)))


def run_composition(tensors, gout, dtype, padding, order, raw, inverse_ao, ao):
    shading = make_shading(ao, inverse_ao)
    cur, prev, input, prev_input = (t.detach().clone().to(dtype) if t is not None else None for t in tensors)
    cur.requires_grad_(True)
    if prev is not None:
        prev.requires_grad_(True)
    out = composition(cur, prev, input, prev_input, padding, shading, order, bool(raw))
    out.backward(gout.to(dtype))
    return out.detach().double(), cur.grad.double(), prev.grad.double() if prev is not None else None


def run_device(tensors, gout, padding, order, raw, inverse_ao, ao):
    shading = make_shading(ao, inverse_ao, device="cuda")
    cur, prev, input, prev_input = (t.detach().cuda() if t is not None else None for t in tensors)
    cur.requires_grad_(True)
    if prev is not None:
        prev.requires_grad_(True)
    out, _, fwd_names = observed(lambda: ops.discriminator_input(cur, prev, input, prev_input, padding=padding, shading=shading, order=order,
                                                                 cur_raw_normal=raw))
    g = gout.cuda()
    _, _, bwd_names = observed(lambda: out.backward(g))
    return (out.detach().cpu(), cur.grad.cpu(), prev.grad.cpu() if prev is not None else None), fwd_names, bwd_names


def check_shape(combination, n, h, w, padding, variants, expect_kernels):
    tensors, planted = operands(combination, n, h, w, padding)
    sets, border = pixel_sets(planted, n, h, w, padding)
    gout = C.uniform(23, n, CHANNELS[combination], h, w)
    bad = []
    for order, raw, inverse_ao, ao in variants:
        # the test's own inputs: every kink CLEAR away outside the planted pixels (cur as the variant shades it, prev always normalised)
        assert kink_clearance(tensors[0], sets["rest"], bool(raw), ao, inverse_ao) >= CLEAR
        if tensors[1] is not None:
            assert kink_clearance(tensors[1], sets["rest"], False, ao, inverse_ao) >= CLEAR
        ref64 = run_composition(tensors, gout, torch.float64, padding, order, raw, inverse_ao, ao)
        ref32 = run_composition(tensors, gout, torch.float32, padding, order, raw, inverse_ao, ao)
        got, fwd_names, bwd_names = run_device(tensors, gout, padding, order, raw, inverse_ao, ao)
        again, _, _ = run_device(tensors, gout, padding, order, raw, inverse_ao, ao)
        if expect_kernels:
            assert fwd_names == [FWD] and bwd_names == [BWD], (fwd_names, bwd_names)
            for a, b in zip(got, again):
                assert (a is None and b is None) or torch.equal(a, b)
        else:
            assert FWD not in fwd_names and BWD not in bwd_names, (fwd_names, bwd_names)
        label = "%s o%d raw%d inv%d ao%.1f" % (combination, order, raw, inverse_ao, ao)
        for k, (what, relative, floor) in enumerate((("values", False, 1e-6), ("grad cur", True, 1e-5), ("grad prev", True, 1e-5))):
            if got[k] is not None:
                bad += compare(label + " " + what, got[k], ref64[k], ref32[k], sets, border, relative, floor)
    assert not bad, bad


def test_planted_pixels_sit_on_their_kinks():
    """The conditions the comparison relies on, asserted on the inputs themselves (CPU): exact values, the same in fp32 and fp64."""
    for n, h, w, padding in SHAPES + [(1, 128, 128, 2)]:
        (cur, prev, _, _), planted = operands("adv26", n, h, w, padding)
        assert set(planted) == {"mask=+1", "mask=-1", "ao=0", "ao=1", "normal=0", "|normal|=5e-8", "n_z=0"}
        for x in (cur, prev):
            at = lambda kind: x.permute(0, 2, 3, 1)[planted[kind]][0]
            assert at("mask=+1")[0] == 1.0 and at("mask=-1")[0] == -1.0 and at("ao=0")[5] == 0.0 and at("ao=1")[5] == 1.0
            assert not at("normal=0")[1:4].any() and at("n_z=0")[3] == 0.0
            for dtype in (torch.float32, torch.float64):
                length = at("|normal|=5e-8")[1:4].to(dtype).norm()
                assert 0 < float(length) < 1e-7 and abs(float(length) - 5e-8) < 1e-14
        inside = torch.zeros(n, h, w, dtype=torch.bool)
        inside[:, padding:h - padding, padding:w - padding] = True
        for m in planted.values():
            assert int(m.sum()) == 1 and bool((m & inside).any())


@pytest.mark.parametrize("combination", list(COMBINATIONS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d_pad%d" % s)
def test_kernels_against_the_fp64_composition(shape, combination):
    n, h, w, padding = shape
    check_shape(combination, n, h, w, padding, VARIANTS, expect_kernels=True)


def test_kernels_at_the_real_plane_size():
    check_shape("adv26", 1, 128, 128, 2, [(0, 1, False, 0.5), (1, 0, True, 1.0)], expect_kernels=True)


@pytest.mark.parametrize("combination", list(COMBINATIONS))
@pytest.mark.parametrize("shape", FALLBACK_SHAPES, ids=lambda s: "%dx%dx%d_pad%d" % s)
def test_refused_shapes_fall_back_and_meet_the_same_bars(shape, combination):
    n, h, w, padding = shape
    tensors, _ = operands(combination, n, h, w, padding)
    cur, prev, input, prev_input = (t.cuda() if t is not None else None for t in tensors)
    assert not ops.discriminator_input_supported(cur, prev, input, prev_input, padding=padding, shading=make_shading(device="cuda"))
    check_shape(combination, n, h, w, padding, [(0, 1, False, 0.5), (1, 0, True, 1.0), (1, 1, False, 0.0)], expect_kernels=False)


def test_predicate():
    shading = make_shading(device="cuda")
    cur = torch.zeros(2, 6, 16, 16, device="cuda")
    prev, input = torch.zeros_like(cur), torch.zeros(2, 5, 16, 16, device="cuda")
    assert ops.discriminator_input_supported(cur, prev, input, input, padding=2, shading=shading)
    assert ops.discriminator_input_supported(cur, prev, padding=0, shading=shading)
    assert ops.discriminator_input_supported(cur, None, input, padding=7, shading=shading)
    assert not ops.discriminator_input_supported(cur, prev, input, input, padding=8, shading=shading)             # 2 pad >= min(H, W)
    assert not ops.discriminator_input_supported(cur, None, None, input, padding=2, shading=shading)              # no term reads that
    assert not ops.discriminator_input_supported(cur.double(), prev.double(), padding=2, shading=shading)
    assert not ops.discriminator_input_supported(cur, prev[:, :, :, :12], padding=2, shading=shading)
    assert not ops.discriminator_input_supported(cur.cpu(), prev.cpu(), padding=2, shading=shading)
    storage = torch.zeros(2 * 6 * 16 * 16 + 1, device="cuda")
    unaligned = storage[1:].view(2, 6, 16, 16)
    assert unaligned.is_contiguous() and unaligned.data_ptr() % 16 == 4
    assert not ops.discriminator_input_supported(unaligned, prev, padding=2, shading=shading)                     # 16-byte accesses
    specular = make_shading(device="cuda")
    specular.enable_specular = True
    assert not ops.discriminator_input_supported(cur, prev, padding=2, shading=specular)
    lib = ops._sr()
    assert lib.isrDiscrInputSupported(2, 16, 16, 2) == 1 and lib.isrDiscrInputSupported(2, 16, 14, 2) == 0
    assert lib.isrDiscrInputSupported(2, 16, 16, 8) == 0 and lib.isrDiscrInputSupported(2, 6, 16, 3) == 0
    # the entry points refuse what the predicate refuses, without a launch
    out = torch.empty(2, 16, 16, 16, device="cuda")
    sh, ao, inv = ops._discr_shading(shading)
    assert lib.isrDiscrInputForward(None, None, unaligned.data_ptr(), prev.data_ptr(), out.data_ptr(), 2, 16, 16, 2, 0, 1, sh, ao, inv, None) == -1
    assert lib.isrDiscrInputForward(None, input.data_ptr(), cur.data_ptr(), prev.data_ptr(), out.data_ptr(), 2, 16, 16, 2, 0, 1, sh, ao, inv, None) == -1


def criterion_names(fused_inputs):
    saved = ops.DISCR_INPUT_FUSED
    ops.DISCR_INPUT_FUSED = fused_inputs
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            _, _, names = observed(lambda: C.check_criterion("cuda", fused=True))
    finally:
        ops.DISCR_INPUT_FUSED = saved
    assert not [str(c.message) for c in caught if issubclass(c.category, RuntimeWarning)], [str(c.message) for c in caught]
    return names


def test_fused_criterion_assembles_its_inputs_with_the_kernels():
    """Case b of the fixture (three adversarial terms): the generator side is one forward and one backward launch per term,
    ``train_discriminator`` two forward launches per term (ground truth, prediction) and no backward (nothing there asks for one)."""
    names = criterion_names(True)
    assert names.count(FWD) == 3 + 3 * 2, names
    assert names.count(BWD) == 3, names


def test_the_switch_takes_the_kernels_out_and_the_criterion_still_matches():
    names = criterion_names(False)
    assert FWD not in names and BWD not in names, names
