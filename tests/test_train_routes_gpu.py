"""Forward and data-gradient convolutions of the training graph (``ops._train_conv``), one launch at a time against fp64, on every
kernel family and kernel form the routing can pick -- and each case asserts the family and the form it ran (train_route_common).

What sets these launches apart from the inference ones of test_conv_gpu.py: transposed and flipped weight images, the 'gate'
epilogue (v = r > 0 ? v : 0, the backward of a ReLU folded into the consumer's data gradient), and the 64 -> 101 data gradient of the
pre-block -- the only launch with more than 64 outputs on the split kernels (two channel groups), and the path back-propagation
through time takes into the previous frame.  The gate operand and the residual are tensors the test supplies, identical on both
sides: no ReLU can switch between device and reference, so the bars are those of one fp32 sum.

Each case runs four launches on one weight [Cout, Cin, 3, 3]:
    forward        relu(conv(x) + b)                and    conv(x) + b + res                   (Cin -> Cout)
    data gradient  conv'(g) where gate > 0, else 0  and    conv'(g) + skip                     (Cout -> Cin)
The routing, restated from ops._train_conv, csrc/sr_conv_split.hip (split_plan) and csrc/sr_conv3x3.hip (isrConv3x3ForwardStrided),
with `out` the output channels of the LAUNCH:
    family   split   out > 8 and W % 4 == 0 and (N ceil(H/8) ceil(W/32) >= 256  or  N ceil(H/2) ceil(W/32) >= 128);  exact otherwise
             bf16    ops.TRAIN_BF16 and out > 8 and more than 8 inputs and N ceil(H/8) ceil(W/32) >= 256
    split    nwg = N ceil(H/8) ceil(W/32) ceil(out/64):  2-row tiles when nwg < 256 (and the 2-row tiling has >= 64 workgroups),
             one workgroup per tile up to 8 x CUs, the persistent streaming form beyond
    exact    big = N ceil(W/32) ceil(H/16) ceil(out/32), small the same with 4-row tiles:  one row per workgroup when big < 384 and
             small <= 160,  4 x 32 tiles when big < 384,  16 x 32 tiles otherwise
The streaming form is reached through the diagnostics build's grid cap (8 and 24 workgroups walk the 288 / 576 tiles): past its
own threshold -- more than 8 x CUs tiles -- the fp64 reference would take too long, and it is the same kernel.

Bars, none of them taken from the kernels under test:
    every launch          max |y - ref| <= 1e-4                 the project's parity bar, operands O(1)
    split and exact       max |y - ref| / max |ref| <= 2e-6 max(1, K / 576),  K = 9 x inputs of the launch: 2e-6 at K = 576 is the bar
                          of test_conv_gpu.py::test_split_operand_accuracy_matches_the_exact_kernel, and the worst-case error of an
                          fp32 sum grows at most linearly with its length
    bf16                  x, w and g rounded to bf16 beforehand: every product is exact in fp32 and only the order of the fp32 sum
                          differs from fp64 -- <= 1e-5 absolute, the fp16 fast mode's bar for the same statement
The measured errors are in profiles/train_routes_errors.md."""
import functools

import pytest
import torch

from train_route_common import ROWS2, ROWSPLIT, STREAM, TILE, TILE4, TILE16, dgrad64, fwd64, observed, record_error

pytestmark = pytest.mark.gpu

TILE_ROWS = {ROWS2: 2, TILE: 8, STREAM: 8, ROWSPLIT: 1, TILE4: 4, TILE16: 16, None: 8}      # None: the bf16 kernel (8 x 32 tiles, not recorded)

# id, mode, (N, H, W), Cin, Cout, (family, kernel) of the forward launches, (family, kernel) of the data-gradient launches.
# Cases that share operands and references follow each other (the cache below holds one set).
CASES = [
    # split, one workgroup per 8 x 32 tile: 12 x 8 = 96 tiles per image, the last tile row 2 rows high, the last tile column 4 wide
    ("tile-64-64", "tile", (3, 90, 228), 64, 64, ("split", TILE), ("split", TILE)),
    ("stream8-64-64", "stream8", (3, 90, 228), 64, 64, ("split", STREAM), ("split", STREAM)),
    ("stream24-64-64", "stream24", (3, 90, 228), 64, 64, ("split", STREAM), ("split", STREAM)),
    ("tile-101-64", "tile", (3, 90, 228), 101, 64, ("split", TILE), ("split", TILE)),                     # data gradient: 576 workgroups
    ("stream8-101-64", "stream8", (3, 90, 228), 101, 64, ("split", STREAM), ("split", STREAM)),
    ("stream24-101-64", "stream24", (3, 90, 228), 101, 64, ("split", STREAM), ("split", STREAM)),
    # six outputs forward: at most 8 outputs never take the split kernels (3 x 8 x 23 = 552 four-row tiles: the 4 x 32 tiling)
    ("tile-64-6", "tile", (3, 90, 228), 64, 6, ("exact", TILE4), ("split", TILE)),
    ("stream8-64-6", "stream8", (3, 90, 228), 64, 6, ("exact", TILE4), ("split", STREAM)),
    ("stream24-64-6", "stream24", (3, 90, 228), 64, 6, ("exact", TILE4), ("split", STREAM)),
    # split, 2-row tiles: 32 tiles of 8 rows, 128 of 2 rows; odd H: the last tile is one row high, the second tile column 4 wide
    ("rows2-64-64", "plain", (4, 31, 36), 64, 64, ("split", ROWS2), ("split", ROWS2)),
    ("rows2-101-64", "plain", (4, 31, 36), 101, 64, ("split", ROWS2), ("split", ROWS2)),
    ("rows2-64-6", "plain", (4, 31, 36), 64, 6, ("exact", ROWSPLIT), ("split", ROWS2)),                   # forward: 4 x 2 x 8 = 64 four-row tiles
    # exact, one row per workgroup (W % 4 != 0 keeps every launch off the split kernels from here on)
    ("rowsplit-64-64", "plain", (1, 9, 7), 64, 64, ("exact", ROWSPLIT), ("exact", ROWSPLIT)),
    ("rowsplit-101-64", "plain", (1, 9, 7), 101, 64, ("exact", ROWSPLIT), ("exact", ROWSPLIT)),
    ("rowsplit-64-6", "plain", (1, 9, 7), 64, 6, ("exact", ROWSPLIT), ("exact", ROWSPLIT)),
    # exact, 4 x 32 tiles: more than 160 of them, fewer than 384 of 16 x 32 (64 outputs: 192 / 48; 101: 384 / 96; 6 at N = 12: 192 / 48)
    ("tile4-64-64", "plain", (6, 30, 33), 64, 64, ("exact", TILE4), ("exact", TILE4)),
    ("tile4-101-64", "plain", (6, 30, 33), 101, 64, ("exact", TILE4), ("exact", TILE4)),
    ("tile4-64-6", "plain", (12, 30, 33), 64, 6, ("exact", TILE4), ("exact", TILE4)),
    # ... and with W % 4 == 0: the tilings' 16-byte epilogue, gate included.  Only a launch with more than 64 outputs gets there on a
    # shape too small for the split kernels (24 tiles, 87 of 2 rows): the 64 -> 101 data gradient, 3 x 15 x 4 = 180 four-row tiles; the
    # last one 2 rows high, the last tile column 28 wide.  (The forward launch, 90 tiles, takes the one-row form.)
    ("tile4-quads-101-64", "plain", (1, 58, 92), 101, 64, ("exact", ROWSPLIT), ("exact", TILE4)),
    # exact, 16 x 32 tiles: at least 384 workgroups (64 outputs: 10 x 5 x 4 x 2 = 400; 101: 800; 6 at N = 20: 400)
    ("tile16-64-64", "plain", (10, 50, 130), 64, 64, ("exact", TILE16), ("exact", TILE16)),
    ("tile16-101-64", "plain", (10, 50, 130), 101, 64, ("exact", TILE16), ("exact", TILE16)),
    ("tile16-64-6", "plain", (20, 50, 130), 64, 6, ("exact", TILE16), ("exact", TILE16)),
    # opt-in bf16 on the tile-form shape; layers with at most 8 inputs or outputs keep their fp32 kernels in that mode
    ("bf16-64-64", "bf16", (3, 90, 228), 64, 64, ("bf16", None), ("bf16", None)),
    ("bf16-101-64", "bf16", (3, 90, 228), 101, 64, ("bf16", None), ("bf16", None)),
    ("bf16-64-6", "bf16", (3, 90, 228), 64, 6, ("exact", TILE4), ("split", TILE)),
]


@functools.lru_cache(maxsize=1)
def _case_data(shape, cin, cout, representable):
    """Operands (fp32, CPU) and the four fp64 references of one shape and channel pair; computed once, never written to."""
    n, h, w = shape
    g = torch.Generator().manual_seed(10000 * cin + 100 * cout + h)
    u = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    t = {"x": u(n, cin, h, w), "w": u(cout, cin, 3, 3) / (3.0 * cin ** 0.5), "b": torch.rand(cout, generator=g) - 0.5, "res": u(n, cout, h, w),
         "g": u(n, cout, h, w), "gate": u(n, cin, h, w), "skip": u(n, cin, h, w)}
    t["gate"][:, ::3] = torch.relu(t["gate"][:, ::3])          # as a ReLU's output: exact zeros; elsewhere signed: negatives close the gate too
    if representable:                                          # the matrix operands in bf16; bias, residual, gate and skip arbitrary fp32
        for k in ("x", "w", "g"):
            t[k] = t[k].bfloat16().float()
    ref = {"fwd relu": fwd64(t["x"], t["w"], t["b"], 'relu', None), "fwd none+res": fwd64(t["x"], t["w"], t["b"], 'none', t["res"]),
           "dgrad gate": dgrad64(t["g"], t["w"], gate=t["gate"]), "dgrad none+skip": dgrad64(t["g"], t["w"], skip=t["skip"])}
    return t, ref


def _compare(case, op, family, kernel, y, ref, inputs):
    """The bars of the module docstring on the last (ragged) tile row, the last tile column and the whole tensor, in that order: a
    failure names the edge."""
    k = 9 * inputs
    rel_bar = None if family == "bf16" else 2e-6 * max(1.0, k / 576.0)
    abs_bar = 1e-5 if family == "bf16" else 1e-4
    y = y.cpu().double()
    assert y.shape == ref.shape
    scale = ref.abs().max().item()
    h, w = ref.shape[2], ref.shape[3]
    r0, c0 = ((h - 1) // TILE_ROWS[kernel]) * TILE_ROWS[kernel], ((w - 1) // 32) * 32
    err = (y - ref).abs()
    for where, e in (("last tile row (%d..)" % r0, err[:, :, r0:]), ("last tile column (%d..)" % c0, err[:, :, :, c0:]), ("whole tensor", err)):
        e = e.max().item()
        print("%s  %s  %s %s  %s: max |y - ref| %.3g, / max |ref| %.3g (bars %.3g, %s)" % (case, op, family, kernel, where, e, e / scale, abs_bar, rel_bar))
        if where == "whole tensor":
            record_error(case, op, family, kernel, e, e / scale, "%.3g abs" % abs_bar if rel_bar is None else "%.3g" % rel_bar)
        assert e <= abs_bar, (case, op, where, e)
        if rel_bar is not None:
            assert e / scale <= rel_bar, (case, op, where, e / scale, rel_bar)


def _run_case(case, shape, cin, cout, representable, fwd, dgrad):
    from isosurfacesuperresolution_amd import ops
    t, ref = _case_data(shape, cin, cout, representable)
    d = {k: v.cuda() for k, v in t.items()}

    def launch(transpose_flip, act, residual, expect):
        family, kernel = expect
        src = d["g"] if transpose_flip else d["x"]
        bias = None if transpose_flip else d["b"]
        y, families, names = observed(lambda: ops._train_conv(src, d["w"], transpose_flip, bias, residual, act))
        assert set(families) == {family}, (case, act, families)
        assert names == ([kernel] if kernel is not None else []), (case, act, names)
        return y

    y = launch(False, 'relu', None, fwd)
    _compare(case, "fwd relu", fwd[0], fwd[1], y, ref["fwd relu"], cin)
    assert (y >= 0).all().item()
    y = launch(False, 'none', d["res"], fwd)
    _compare(case, "fwd none+res", fwd[0], fwd[1], y, ref["fwd none+res"], cin)

    gated = launch(True, 'gate', d["gate"], dgrad)
    _compare(case, "dgrad gate", dgrad[0], dgrad[1], gated, ref["dgrad gate"], cout)
    closed = d["gate"] <= 0
    assert closed[:, ::3].any().item() and closed[:, 1::3].any().item() and not closed.all().item()      # exact zeros and negatives
    assert (gated[closed] == 0).all().item(), (case, "the gate let %d values through" % int((gated[closed] != 0).sum().item()))
    ungated = launch(True, 'none', None, dgrad)                # the same launch without the gate, on the same route
    assert (ungated[closed] != 0).any().item()
    assert torch.equal(gated, torch.where(d["gate"] > 0, ungated, torch.zeros_like(ungated))), (case, "the gate changed a value it let through")
    y = launch(True, 'none', d["skip"], dgrad)
    _compare(case, "dgrad none+skip", dgrad[0], dgrad[1], y, ref["dgrad none+skip"], cout)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_train_conv_matches_fp64_on_the_route_it_names(case, request):
    from isosurfacesuperresolution_amd import ops
    name, mode, shape, cin, cout, fwd, dgrad = case
    assert not ops.TRAIN_BF16 and ops.TRAIN_SPLIT and ops.FLOP_TALLY is None and not ops.profile_is_on()
    if mode in ("stream8", "stream24"):
        lib = request.getfixturevalue("diag_lib")
        try:
            lib.isrDebugSetSplitSmall(0)
            lib.isrDebugSetSplitSlots(int(mode[6:]))
            _run_case(name, shape, cin, cout, False, fwd, dgrad)
        finally:
            lib.isrDebugSetSplitSlots(0)
            lib.isrDebugSetSplitSmall(1)
        assert ops.debug_switches() == 0
    elif mode == "bf16":
        ops.TRAIN_BF16 = True
        try:
            _run_case(name, shape, cin, cout, True, fwd, dgrad)
        finally:
            ops.TRAIN_BF16 = False
    else:
        _run_case(name, shape, cin, cout, False, fwd, dgrad)
    assert not ops.TRAIN_BF16 and ops.FLOP_TALLY is None and not ops.profile_is_on()


def test_the_cases_cover_every_form_with_the_pre_block_data_gradient():
    """The 64 -> 101 data gradient (weight [64, 101, 3, 3]) on every split form and every exact form, and all three channel pairs on each."""
    for kernel in (ROWS2, TILE, STREAM, ROWSPLIT, TILE4, TILE16):
        pairs = {(c[3], c[4]) for c in CASES if c[6][1] == kernel}
        assert (101, 64) in pairs, kernel
        assert pairs >= {(64, 64), (101, 64), (64, 6)}, (kernel, pairs)
    assert {(c[3], c[4]) for c in CASES if c[6][0] == "bf16"} == {(64, 64), (101, 64)}
