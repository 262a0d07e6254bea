"""What tests/test_discr_input_cpu.py and tests/test_discr_input_gpu.py share: the composition that ``ops.discriminator_input`` replaces,
written out from ``ScreenSpaceShading`` and ``LossNetUnshaded.pad`` as the criterion ran it before the kernels, the loss shader of the
recorded cases, and operands whose kinks are under control.

The kinks of the map (places where its derivative jumps): ``light . normal`` against 0 (``abs``), ``mask / 2 + 1 / 2``, the AO argument
(``ao`` or ``1 - ao``) and the pre-clamp colour against 0 and 1 (``clamp``), ``|normal|`` against 1e-7 (``normalize``).  ``field6`` draws
uniform operands and moves every value that comes within ``CLEAR`` of a kink; ``plant`` then writes a few pixels EXACTLY onto kinks,
with values that are the same numbers in fp32 and fp64, so that both precisions take the same branch there."""
import numpy as np
import torch

import gan_common as C
from isosurfacesuperresolution_amd import losses
from isosurfacesuperresolution_amd.utils import ScreenSpaceShading

COMBINATIONS = {"adv26": (True, True, True), "tgan16": (False, False, True), "sgan13": (True, False, False)}      # input, prev_input, prev
CHANNELS = {"adv26": 26, "tgan16": 16, "sgan13": 13}
CLEAR = 1e-3
TINY = float(np.float32(5e-8))          # |normal| below normalize's 1e-7, the same number in fp32 and fp64


def make_shading(ao=0.5, inverse_ao=False, device="cpu"):
    """The criterion's loss shader (lossnet_unshaded.py:116-126 with the options of gan_common.options): light (0, 0, 1), ambient 0.1,
    diffuse 0.9, white material, black background, no specular."""
    sh = ScreenSpaceShading(device)
    sh.fov(30)
    sh.ambient_light_color(np.array([0.1] * 3))
    sh.diffuse_light_color(np.array([0.9] * 3))
    sh.specular_light_color(np.array([0.0] * 3))
    sh.specular_exponent(16)
    sh.enable_specular = False
    sh.light_direction(np.array([0.0, 0.0, 1.0]))
    sh.material_color(np.array([1.0, 1.0, 1.0]))
    sh.ambient_occlusion(ao)
    sh.inverse_ao = inverse_ao
    return sh


def composition(cur, prev, input, prev_input, padding, shading, order, cur_raw_normal):
    """normalise, shade, concatenate in the side's order (0: colour before ao, the generator's; 1: ao before colour,
    train_discriminator's), zero the border; any floating-point type."""
    pad, norm = losses.LossNetUnshaded.pad, ScreenSpaceShading.normalize

    def part(t, raw):
        mask, normal, ao = t[:, 0:1], norm(t[:, 1:4], dim=1), t[:, 5:6]
        color = shading(t) if raw else shading(torch.cat([mask, normal, t[:, 4:6]], dim=1))
        return pad(torch.cat([mask, normal, color, ao] if order == 0 else [mask, normal, ao, color], dim=1), padding)

    parts = [pad(t, padding) for t in (input, prev_input) if t is not None]
    parts.append(part(cur, cur_raw_normal))
    if prev is not None:
        parts.append(part(prev, False))
    return torch.cat(parts, dim=1)


def field6(seed, n, h, w):
    """[n, 6, h, w] fp32: mask in [-1.5, 1.5] (both clamps of mask / 2 + 1 / 2 are taken), normal in [-1, 1]^3, depth in [0, 1], ao in
    [-0.5, 1.5] (both clamps of the AO argument), every kink at least CLEAR away (``kink_clearance`` measures it)."""
    rs = np.random.RandomState(seed)
    x = np.empty((n, 6, h, w), dtype=np.float32)
    x[:, 0] = rs.uniform(-1.5, 1.5, (n, h, w))
    x[:, 1:4] = rs.uniform(-1.0, 1.0, (n, 3, h, w))
    x[:, 4] = rs.uniform(0.0, 1.0, (n, h, w))
    x[:, 5] = rs.uniform(-0.5, 1.5, (n, h, w))
    m, nx, ny, nz, ao = x[:, 0], x[:, 1], x[:, 2], x[:, 3], x[:, 5]
    # the pre-clamp colour is t (0.1 + 0.9 |l . n|) aof, t = clamp(mask / 2 + 1 / 2), aof = s clamp(a) + 1 - s: it stays CLEAR of 0 where
    # t and a are either clamped to 0 (the colour is then exactly 0) or at least 0.12 (0.12 x 0.1 x 0.12 = 1.44 CLEAR) ...
    m[(np.abs(m - 1.0) < 4 * CLEAR) | ((m > -1.0 - 4 * CLEAR) & (m < -1.0 + 0.24))] = 0.25      # mask / 2 + 1 / 2: 2 CLEAR from 0 and 1
    ao[((ao > -2 * CLEAR) & (ao < 0.12)) | ((ao > 0.88) & (ao < 1.0 + 2 * CLEAR))] = 0.5        # ao and 1 - ao
    nz[(np.abs(nz) < 4 * CLEAR) | (np.abs(nz) > 0.99)] = 0.5        # light . normal = n_z (raw) or n_z / |n|: away from 0 ...
    nx[np.sqrt(nx * nx + ny * ny) < 0.2 * np.abs(nz)] = 0.5         # ... and |n_z| / |n| <= 0.981: the colour stays below 0.99
    return torch.from_numpy(x)


def plant(x, padding):
    """Writes the exact kink values into interior pixels of image 0 of ``x`` [n, 6, h, w] (in place) -> {kind: [n, h, w] bool mask}.
    One kind per pixel where the interior has seven pixels, else (a 2 x 2 interior) grouped on four."""
    n, _, h, w = x.shape
    pixels = [(yy, xx) for yy in range(padding, h - padding) for xx in range(padding, w - padding)]
    values = {"mask=+1": {0: 1.0}, "mask=-1": {0: -1.0}, "ao=0": {5: 0.0}, "ao=1": {5: 1.0}, "normal=0": {1: 0.0, 2: 0.0, 3: 0.0},
              "|normal|=5e-8": {1: 0.0, 2: 0.0, 3: TINY}, "n_z=0": {3: 0.0}}
    if len(pixels) >= 7:
        step = len(pixels) // 7                                     # spread over the interior: several rows, several quads
        groups = [((kind,), pixels[k * step]) for k, kind in enumerate(values)]
    else:
        assert len(pixels) >= 4
        groups = [(("mask=+1", "ao=0", "n_z=0"), pixels[0]), (("mask=-1", "ao=1"), pixels[1]), (("normal=0",), pixels[2]),
                  (("|normal|=5e-8",), pixels[3])]
    masks = {}
    for kinds, (yy, xx) in groups:
        for kind in kinds:
            for channel, value in values[kind].items():
                x[0, channel, yy, xx] = value
            masks[kind] = torch.zeros(n, h, w, dtype=torch.bool)
            masks[kind][0, yy, xx] = True
    return masks


def kink_clearance(x, where, raw_normal, ao_strength, inverse_ao):
    """Smallest distance of a kink quantity from its kink over the pixels ``where`` [n, h, w] of ``x`` [n, 6, h, w], in fp64.  A
    pre-clamp colour that is EXACTLY 0 (a factor clamped to 0: the same 0 in every precision) does not count."""
    v = x.double().permute(0, 2, 3, 1)[where]
    if v.numel() == 0:
        return float("inf")
    m, nrm, ao = v[:, 0], v[:, 1:4], v[:, 5]
    length = nrm.norm(dim=1)
    ndl = nrm[:, 2] if raw_normal else nrm[:, 2] / length.clamp_min(1e-7)
    t = m * 0.5 + 0.5
    a = 1.0 - ao if inverse_ao else ao
    colour = t.clamp(0, 1) * (float(np.float32(0.1)) + float(np.float32(0.9)) * ndl.abs()) * (ao_strength * a.clamp(0, 1) + (1.0 - ao_strength))
    colour = colour[colour != 0]
    distances = [ndl.abs(), t.abs(), (t - 1).abs(), a.abs(), (a - 1).abs(), (length - 1e-7).abs(), colour.abs(), (colour - 1).abs()]
    return min(float(d.min()) for d in distances if d.numel())


def operands(combination, n, h, w, padding, seed=7):
    """(cur, prev, input, prev_input) fp32 on the CPU, parts the combination lacks None, and the planted kinds' pixel masks (cur and prev
    are planted alike)."""
    has_input, has_prev_input, has_prev = COMBINATIONS[combination]
    cur = field6(seed, n, h, w)
    planted = plant(cur, padding) if 2 * padding < min(h, w) else {}
    prev = None
    if has_prev:
        prev = field6(seed + 1, n, h, w)
        if planted:
            plant(prev, padding)
    input = C.uniform(seed + 2, n, 5, h, w) if has_input else None
    prev_input = C.uniform(seed + 3, n, 5, h, w) if has_prev_input else None
    return (cur, prev, input, prev_input), planted


def pixel_sets(planted, n, h, w, padding):
    inside = torch.zeros(n, h, w, dtype=torch.bool)
    if 2 * padding < min(h, w):
        inside[:, padding:h - padding, padding:w - padding] = True
    any_planted = torch.zeros(n, h, w, dtype=torch.bool)
    for m in planted.values():
        any_planted |= m
    return dict(planted, rest=inside & ~any_planted), ~inside


def compare(label, got, ref64, ref32, sets, border, relative, floor, record=None):
    """The comparison rule of the element-wise training kernels' tests (test_discr_input_gpu.py, test_train_pointwise_gpu.py).  Per pixel set: the largest |got - fp64| against max(4 x largest |fp32 - fp64|, floor), both relative to the set's largest |fp64|
    for a gradient (``relative``); border pixels exactly 0.  -> the sets that miss.  ``record(label, kind, error, own, bar)`` is called
    for every set, if given."""
    at = lambda t, m: t.permute(0, 2, 3, 1)[m]
    assert not at(got, border).any(), "%s: a border pixel is not 0" % label
    bad = []
    for kind, m in sets.items():
        if not m.any():
            continue
        r = at(ref64, m)
        scale = float(r.abs().max()) if relative else 1.0
        err, own = float((at(got, m).double() - r).abs().max()), float((at(ref32, m) - r).abs().max())
        bar = max(4.0 * own, floor * scale)
        print("%-34s %-14s error %.3e  fp32-vs-fp64 %.3e  bar %.3e  (largest |value| %.3e)" % (label, kind, err, own, bar, float(r.abs().max())))
        if record is not None:
            record(label, kind, err, own, bar)
        if not err <= bar:
            bad.append((label, kind, err, bar))
    return bad
