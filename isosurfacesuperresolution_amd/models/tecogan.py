"""TecoGAN generator (Chu et al.) as the reference's trainer and viewer accept it beside EnhanceNet.

Same constructor, stored attributes, sub-module names and ``state_dict`` keys as ``SuperresolutionNetwork/models/tecogan.py``
(``preblock.0``, ``blocks.{i}.{0,2}``, ``postblock.{0,2,4}``), so reference checkpoints -- state dicts and pickled whole objects --
load; the forward pass is written against ``ops`` so that on an MI355X every layer is one fused HIP launch: the 3x3 convolutions
``ops.conv3x3`` (bias + LeakyReLU / residual add in the epilogue), the two learned x2 upsamplings ``ops.conv_transpose3x3_s2``.

Architecture (tecogan.py:41-62): pre: conv(Cin -> 64) + LeakyReLU; ``numResidualLayers`` x [conv + LeakyReLU, conv] with skip; post:
ConvTranspose2d(64, 64, 3, stride 2, padding 1, output_padding 1) + LeakyReLU, twice; conv(64 -> Cout) + LeakyReLU.  ``nn.LeakyReLU()``:
slope 0.01.  Initialisation: PyTorch defaults (the reference leaves its orthogonal initialisation commented out, :23).
Reconstruction (:25-39): ``'residual'`` adds the resized input channels ``channel_mask`` -- GATHERED by index, and added to the WHOLE
output: there is no concatenation, so a residual TecoGAN needs ``len(channel_mask) == output_channels`` (the colour family: [0, 1, 2]
with three outputs; the unshaded family, mask [0..4] with six outputs, exists only with ``reconType='direct'``).

A pickled reference object carries only ``upscale_factor, upsample, recon_type, num_residual_layers, channel_mask`` (unpickling
bypasses ``__init__``): nothing else is read here; channel counts come from the convolutions.  Training runs on the HIP path too:
under autograd ``ops.conv_transpose3x3_s2`` is one node on the transposed convolution's own forward, phase-gradient and data-gradient
kernels, its weight gradient deferred like every other layer's (``train.backward``)."""
import torch.nn as nn
import torch.nn.functional as F

from .. import ops

SLOPE = 0.01            # nn.LeakyReLU()'s default


class TecoGAN(nn.Module):
    def __init__(self, upscale_factor, input_channels, channel_mask, output_channels, opt):
        super().__init__()
        assert upscale_factor == 4
        self.upscale_factor = upscale_factor
        self.upsample = opt.upsample
        self.recon_type = opt.reconType
        self.num_residual_layers = opt.numResidualLayers
        self.channel_mask = channel_mask
        self._build(input_channels, output_channels)

    def _build(self, cin, cout):
        def conv(i, o):
            return nn.Conv2d(i, o, 3, padding=1)

        def up():
            return nn.ConvTranspose2d(64, 64, 3, stride=2, padding=1, output_padding=1)

        self.preblock = nn.Sequential(conv(cin, 64), nn.LeakyReLU())
        self.blocks = nn.ModuleList([nn.Sequential(conv(64, 64), nn.LeakyReLU(), conv(64, 64)) for _ in range(self.num_residual_layers)])
        self.postblock = nn.Sequential(up(), nn.LeakyReLU(), up(), nn.LeakyReLU(), conv(64, cout), nn.LeakyReLU())

    # ------------------------------------------------------------------ forward
    def _recon_image(self, inputs, outputs):
        if self.recon_type != 'residual':
            return outputs, outputs
        mask = list(self.channel_mask)
        k = len(mask)
        if k != outputs.shape[1]:
            # the reference adds the resized masked input to the WHOLE output (tecogan.py:30-35)
            raise RuntimeError("TecoGAN residual reconstruction: the size of the masked input (%d channels) must match the size of the "
                               "output (%d channels)" % (k, outputs.shape[1]))
        if mask == list(range(k)) and self.upsample == 'bilinear' and ops.recon_residual_supported(outputs, inputs, k):
            return ops.recon_residual(outputs, inputs, k), outputs          # slice + resize + add as one HIP launch
        resized = F.interpolate(inputs[:, mask, :, :], size=[outputs.shape[2], outputs.shape[3]], mode=self.upsample)
        return resized + outputs, outputs

    def forward_features(self, inputs, after_trunk=None):
        """The convolutional part only: the tensor ``_recon_image`` receives (the fused frame pipeline folds the reconstruction into
        its finishing kernel).  ``after_trunk``: called once the low-resolution residual blocks have been enqueued (the frame pipeline
        starts the next frame's ray-march there, beside the high-resolution layers)."""
        c = ops.conv3x3
        pre = self.preblock[0]
        f = c(inputs, pre.weight, pre.bias, act='leaky', slope=SLOPE)
        for block in self.blocks:
            t = c(f, block[0].weight, block[0].bias, act='leaky', slope=SLOPE)
            f = c(t, block[2].weight, block[2].bias, residual=f)
        if after_trunk is not None:
            after_trunk()
        p = self.postblock
        f = ops.conv_transpose3x3_s2(f, p[0].weight, p[0].bias, act='leaky', slope=SLOPE)
        f = ops.conv_transpose3x3_s2(f, p[2].weight, p[2].bias, act='leaky', slope=SLOPE)
        return c(f, p[4].weight, p[4].bias, act='leaky', slope=SLOPE)

    def forward(self, inputs):
        return self._recon_image(inputs, self.forward_features(inputs))
