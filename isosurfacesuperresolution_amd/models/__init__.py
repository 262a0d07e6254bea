"""Generator networks.  ``createNetwork`` mirrors ``SuperresolutionNetwork/models/__init__.py:21-49``:
EnhanceNet, TecoGAN (its stride-2 transposed convolutions on ``ops.conv_transpose3x3_s2``) and RCAN (its
channel attention on ``ops.channel_attention_residual``, its pixel-shuffle tail on ``ops.pixel_shuffle4_conv``; the colour family only,
as in the reference) run on the HIP kernels; SubpixelNet (5x5 convolutions) is out of scope and raises."""
from .enhancenet import EnhanceNet
from .rcan import RCAN
from .tecogan import TecoGAN
from .videotools import VideoTools


def createNetwork(name, upscale_factor, input_channels, channel_mask, output_channels, additional_opt):
    print('upscale_factor:', upscale_factor)
    print('input_channels:', input_channels)
    print('channel_mask:', channel_mask)
    print('output_channels:', output_channels)
    key = name.lower()
    if key == 'enhancenet':
        return EnhanceNet(upscale_factor, input_channels, channel_mask, output_channels, additional_opt)
    if key == 'tecogan':
        return TecoGAN(upscale_factor, input_channels, channel_mask, output_channels, additional_opt)
    if key == 'rcan':
        return RCAN(upscale_factor, input_channels, channel_mask, output_channels, additional_opt)
    if key == 'subpixelnet':
        raise NotImplementedError("generator '%s' is outside the accelerated hot path" % name)
    raise ValueError('Unknown model %s' % name)
