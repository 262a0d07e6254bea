"""Host definition of the split-operand weight image (csrc/sr_split_prepare.hip), in plain torch on CPU tensors: what the bytes of an
image must be, written down independently of the library.

    unit 0                                                        header { 2^S, 2^-S, S, 0 }, S = 13 - floor(log2 max|w|) clamped to +-100,
                                                                  0 for a maximum that is zero or not below 3e38
    unit 1 + (((tap ksteps + s) 2 + part) 2 + h) rowPad + row     eight fp16: part (0 hi, 1 lo) of w 2^S at k = 16 s + 8 h + e
    third plane, behind those: ((tap ksteps + s) 2 + h) rowPad + row     fp16(hi 2^-11)

hi = fp16(v), lo = fp16(v - float(hi)) with v = w 2^S in fp32; ksteps = ceil(k / 16), rowPad = rows rounded up to 32, zeros beyond."""
import math
import struct

import torch


def scale_exponent(mx):
    """The scale rule, of the fp32 maximum ``mx`` (a Python float)."""
    if not (mx > 0.0 and mx < 3.0e38):        # zero, inf, NaN
        return 0
    return max(-100, min(100, 13 - (math.frexp(mx)[1] - 1)))


def header(S):
    return struct.pack("<ffiI", 2.0 ** S, 2.0 ** -S, S, 0)


def split_image(w, row_dim, flip, third):
    """Image bytes (uint8 tensor) of the fp32 CPU tensor w [d0][d1][3][3]: rows are dimension ``row_dim``, k the other; ``flip``: tap
    8 - tap of the source; ``third``: with the hi 2^-11 plane."""
    w = w.detach().to(torch.float32).cpu()
    S = scale_exponent(w.abs().max().item())
    m = w.reshape(w.shape[0], w.shape[1], 9)
    if row_dim == 1:
        m = m.transpose(0, 1)
    if flip:
        m = m.flip(2)
    rows, k = m.shape[0], m.shape[1]
    ksteps, row_pad = (k + 15) // 16, (rows + 31) // 32 * 32
    v = torch.zeros(row_pad, ksteps * 16, 9, dtype=torch.float32)
    v[:rows, :k] = m * torch.tensor(2.0 ** S, dtype=torch.float32)          # a power of two: exact (or the fp32 rounding the kernel has too)
    hi = v.to(torch.float16)
    lo = (v - hi.to(torch.float32)).to(torch.float16)
    # [row][s][h][e][tap] -> [tap][s][h][row][e]
    order = lambda t: t.reshape(row_pad, ksteps, 2, 8, 9).permute(4, 1, 2, 0, 3)
    planes = torch.stack([order(hi), order(lo)], dim=2).contiguous()         # [tap][s][part][h][row][e]
    parts = [torch.frombuffer(bytearray(header(S)), dtype=torch.uint8), planes.view(torch.uint8).reshape(-1)]
    if third:
        hs = (hi * torch.tensor(2.0 ** -11, dtype=torch.float16))            # an fp16 product, rounded once (subnormals kept)
        parts.append(order(hs).contiguous().view(torch.uint8).reshape(-1))
    return torch.cat(parts)


# the four images the library makes: (row dimension, flip, third plane)
CONV_FORWARD, CONV_DGRAD, CONVT_FORWARD, CONVT_DGRAD = (0, False, True), (1, True, True), (1, False, False), (0, False, False)
