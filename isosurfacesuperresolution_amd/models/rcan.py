"""RCAN generator (Zhang et al., "Image Super-Resolution Using Very Deep Residual Channel Attention Networks") as the reference's
trainer accepts it beside EnhanceNet and TecoGAN.

Same constructor, stored attributes, sub-module names and ``state_dict`` keys as ``SuperresolutionNetwork/models/rcan.py``
(``net.pre``, ``net.rir.blocks.{g}.blocks.{b}.pre.{0,2}``, ``net.rir.blocks.{g}.blocks.{b}.ca.{downscaling,upscaling}``,
``net.rir.blocks.{g}.post``, ``net.rir.post``, ``net.post``), so state dicts trained with the reference load
(``RCAN.from_state_dict``).  The block classes are defined at MODULE level here -- the keys do not depend on class names, and a whole
object of this package's RCAN then pickles without ``getattr`` and loads through the restricted unpickler of
``inference.LoadedModel``; the reference's own whole-object RCAN pickles reach its NESTED classes through ``__builtin__ getattr``,
which that unpickler refuses by design.

Architecture (rcan.py:17-110; the counts are constants there, ``opt`` is never read): pre: conv(Cin -> 64); residual in residual:
10 groups x 20 blocks, block = x + ca(conv(LeakyReLU(conv(x)))), group = post(blocks(x)) + x, whole = post(groups(x)) + x;
channel attention ca(t) = t * sigmoid(up(leaky_relu(down(mean_hw(t))))) with ``nn.Linear(64, 4)`` / ``nn.Linear(4, 64)``;
up: PixelShuffle(4), 64 -> 4 channels; post: conv(4 -> Cout).  Every LeakyReLU has slope 0.01.
Forward (:112-121): ``(clamp(out, 0, 1), out - bilinear(inputs[:, channel_mask]))`` -- the masked channels GATHERED by index, no
residual reconstruction; the subtraction needs ``len(channel_mask) == output_channels``, so the network exists for the colour family
(three outputs, mask [0, 1, 2]) only.

On an MI355X every convolution is one ``ops.conv3x3`` launch (bias + LeakyReLU / residual in the epilogue), every block's attention
two launches (``ops.channel_attention_residual``) and the tail one (``ops.pixel_shuffle4_conv``); under autograd the same launches
run forward and each of the two has its own backward kernels (at most three launches per block, three for the tail)."""
import re

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops

SLOPE = 0.01            # nn.LeakyReLU()'s and F.leaky_relu's default


def _conv(i, o):
    return nn.Conv2d(i, o, 3, padding=1)


class ChannelAttentionBlock(nn.Module):
    def __init__(self, num_channels, reduced_channels):
        super().__init__()
        self.downscaling = nn.Linear(num_channels, reduced_channels)
        self.upscaling = nn.Linear(reduced_channels, num_channels)

    def forward(self, x):
        return ops.channel_attention_residual(torch.zeros_like(x), x, self.downscaling.weight, self.downscaling.bias,
                                              self.upscaling.weight, self.upscaling.bias, slope=SLOPE)


class ResidualChannelAttentionBlock(nn.Module):
    def __init__(self, num_channels, reduced_channels):
        super().__init__()
        self.pre = nn.Sequential(_conv(num_channels, num_channels), nn.LeakyReLU(inplace=True), _conv(num_channels, num_channels))
        self.ca = ChannelAttentionBlock(num_channels, reduced_channels)

    def forward(self, x, gates=None):
        a, b, ca = self.pre[0], self.pre[2], self.ca
        t = ops.conv3x3(x, a.weight, a.bias, act='leaky', slope=SLOPE)
        t = ops.conv3x3(t, b.weight, b.bias)
        # the range guard's word of the second convolution is armed again for the gate launch: one word per block (ops._arm_range)
        out = ops.channel_attention_residual(x, t, ca.downscaling.weight, ca.downscaling.bias, ca.upscaling.weight, ca.upscaling.bias,
                                             slope=SLOPE, return_gate=gates is not None, range_key=id(b.weight))
        if gates is not None:
            gates.append(out[1])
            return out[0]
        return out


class ResGroup(nn.Module):
    def __init__(self, num_channels, reduced_channels, num_blocks):
        super().__init__()
        self.blocks = nn.ModuleList([ResidualChannelAttentionBlock(num_channels, reduced_channels) for _ in range(num_blocks)])
        self.post = _conv(num_channels, num_channels)

    def forward(self, x, gates=None):
        f = x
        for block in self.blocks:
            f = block(f, gates)
        return ops.conv3x3(f, self.post.weight, self.post.bias, residual=x)


class RIR(nn.Module):
    def __init__(self, num_channels, reduced_channels, num_groups, num_blocks):
        super().__init__()
        self.blocks = nn.ModuleList([ResGroup(num_channels, reduced_channels, num_blocks) for _ in range(num_groups)])
        self.post = _conv(num_channels, num_channels)

    def forward(self, x, gates=None):
        f = x
        for group in self.blocks:
            f = group(f, gates)
        return ops.conv3x3(f, self.post.weight, self.post.bias, residual=x)


class RCAN(nn.Module):
    def __init__(self, upscale_factor, input_channels, channel_mask, output_channels, opt):
        super().__init__()
        assert upscale_factor == 4
        if len(channel_mask) != output_channels:
            raise NotImplementedError("RCAN with %d masked input channels and %d outputs: the reference's own forward cannot run this "
                                      "configuration (it subtracts the resized masked input from the whole output, rcan.py:117); "
                                      "the network exists for the colour family only" % (len(channel_mask), output_channels))
        self.upscale_factor = upscale_factor
        self.upsample = 'pixelShuffle'
        self.num_blocks_g = int(getattr(opt, 'rcanGroups', 10) or 10)        # (optional fields: tests build small networks)
        self.num_blocks_b = int(getattr(opt, 'rcanBlocks', 20) or 20)
        self.num_channels = 64
        self.channel_downscaling = 16
        self.reduced_channels = self.num_channels // self.channel_downscaling
        self.channel_mask = channel_mask
        c, r = self.num_channels, self.reduced_channels
        self.net = nn.ModuleDict({
            'pre': _conv(input_channels, c),
            'rir': RIR(c, r, self.num_blocks_g, self.num_blocks_b),
            'up': nn.PixelShuffle(upscale_factor),
            'post': _conv(c // upscale_factor ** 2, output_channels)})

    @classmethod
    def from_state_dict(cls, state_dict, channel_mask):
        """A network built for and filled with ``state_dict`` (the loading route for weights trained with the reference, together
        with ``LoadedModel.from_model``): input / output channels and the group and block counts come from the keys and shapes."""
        groups, blocks = set(), set()
        for key in state_dict:
            m = re.match(r"net\.rir\.blocks\.(\d+)\.blocks\.(\d+)\.", key)
            if m:
                groups.add(int(m.group(1))); blocks.add(int(m.group(2)))
        if not groups or 'net.pre.weight' not in state_dict or 'net.post.weight' not in state_dict:
            raise ValueError("not an RCAN state dict")

        class _Counts:
            rcanGroups, rcanBlocks = max(groups) + 1, max(blocks) + 1
        net = cls(4, state_dict['net.pre.weight'].shape[1], list(channel_mask), state_dict['net.post.weight'].shape[0], _Counts)
        net.load_state_dict(state_dict)
        return net

    # ------------------------------------------------------------------ forward
    def forward_features(self, inputs, after_trunk=None, gates=None):
        """The 64-channel tensor after ``net.rir`` (the input of the pixel-shuffle tail).  ``after_trunk``: called once the
        low-resolution layers have been enqueued (the frame pipeline starts the next frame's ray-march there).  ``gates``: a list
        that receives every block's gate vector [N, 64] in network order."""
        pre = self.net['pre']
        f = ops.conv3x3(inputs, pre.weight, pre.bias)
        f = self.net['rir'](f, gates)
        if after_trunk is not None:
            after_trunk()
        return f

    def forward(self, inputs):
        post = self.net['post']
        raw = ops.pixel_shuffle4_conv(self.forward_features(inputs), post.weight, post.bias)
        mask = list(self.channel_mask)
        # consecutive channels (the colour family's [0, 1, 2]) as a slice: the same values without the index tensor that a list builds on
        # the host -- a copy to the device, which a HIP graph capture of the training step (train.GraphedTrainStep) does not allow
        masked = inputs[:, mask[0]:mask[-1] + 1] if mask == list(range(mask[0], mask[0] + len(mask))) else inputs[:, mask, :, :]
        residual = raw - F.interpolate(masked, size=(raw.shape[2], raw.shape[3]), mode='bilinear')
        return torch.clamp(raw, 0, 1), residual
