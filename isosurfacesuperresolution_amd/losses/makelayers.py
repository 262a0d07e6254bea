"""``_make_layers``: the convolution stack of the discriminators (``SuperresolutionNetwork/losses/makelayers.py``) and how it runs here.

A configuration is a list of output channel counts; ``(channels, stride)`` gives a layer a stride and ``'M'`` is a 2x2 max pooling.  Every
convolution is 3x3 with padding 1 and is followed by ``nn.LeakyReLU()`` (slope 0.01).  The modules sit in one ``nn.Sequential`` in the
reference's order, so the ``state_dict`` keys (``0.weight``, ``2.weight``, ...) are the reference's; ``layer_map`` names the convolutions
``conv<block>_<index>`` and the poolings ``pool<block>`` as the reference does.

``run_layers`` is the forward of such a stack on this package's kernels: a convolution and the LeakyReLU behind it are ONE call of
``ops.conv3x3`` (stride 1) or ``ops.conv3x3_s2`` (stride 2) with the activation in the epilogue; on CPU tensors both are the torch
definition, i.e. what ``nn.Sequential`` computes."""
import math

import torch.nn as nn

from .. import ops


def _make_layers(cfg, batch_norm=False, batch_norm_params=None, in_channels=3):
    if batch_norm:
        # (the reference's own batch-norm branch names a LossBuilder attribute that makelayers.py never imports)
        raise NotImplementedError("_make_layers: batch normalisation is outside the accelerated hot path")
    layers, layer_map = [], {}
    block, index = 1, 1
    for v in cfg:
        if v == 'M':
            pool = nn.MaxPool2d(kernel_size=2, stride=2)
            layers.append(pool)
            layer_map['pool%d' % block] = pool
            block, index = block + 1, 1
            continue
        channels, stride = v if isinstance(v, tuple) else (v, 1)
        conv = nn.Conv2d(in_channels, channels, kernel_size=3, stride=stride, padding=1)
        layer_map['conv%d_%d' % (block, index)] = conv
        index += 1
        layers += [conv, nn.LeakyReLU()]
        in_channels = channels
    return nn.Sequential(*layers), layer_map


def run_layers(features, x):
    """``features(x)`` for a stack built by ``_make_layers``, each convolution + LeakyReLU pair as one fused layer."""
    mods = list(features)
    k = 0
    while k < len(mods):
        m = mods[k]
        if isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and m.padding == (1, 1) and m.stride in ((1, 1), (2, 2)) \
                and k + 1 < len(mods) and isinstance(mods[k + 1], nn.LeakyReLU):
            conv = ops.conv3x3 if m.stride == (1, 1) else ops.conv3x3_s2
            x = conv(x, m.weight, m.bias, act='leaky', slope=mods[k + 1].negative_slope)
            k += 2
        else:
            x = m(x)
            k += 1
    return x


class HalvingDiscriminator(nn.Module):
    """What the reference's two EnhanceNet discriminators share (``enhancenetsmall.py``, ``enhancenetlarge.py``): input
    [B, input_channels, resolution, resolution], resolution a power of two; while the image is larger than 4 x 4 the channel count
    doubles (16, 32, 64, ...) and a block of ``block(channels)`` layers, the last one of stride 2, halves it; then ``Linear(C * 16, 1024)``,
    LeakyReLU, ``Linear(1024, 1)``: one logit per image (the sigmoid sits in the loss).  Attributes (``features``, ``classifier``,
    ``resolution``, ``input_channels``), ``state_dict`` keys and initialisation (``:39-48`` of either file: convolutions N(0, 2 / (9 Cout)),
    Linear N(0, 0.01), biases zero, drawn in module order) are the reference's.  ``forward`` runs the convolutions on ``ops.conv3x3`` /
    ``ops.conv3x3_s2`` (``run_layers``) and the classifier on ``nn.Linear``."""

    @staticmethod
    def block(channels):
        raise NotImplementedError

    def __init__(self, resolution, input_channels):
        super().__init__()
        self.resolution = resolution
        self.input_channels = input_channels
        assert (resolution & (resolution - 1)) == 0, "resolution is not a power of two: %d" % resolution
        config, channels = [], 8
        while resolution > 4:
            channels, resolution = channels * 2, resolution // 2
            config += self.block(channels)
        assert resolution == 4
        self.features, _ = _make_layers(config, False, in_channels=input_channels)
        self.classifier = nn.Sequential(nn.Linear(channels * 4 * 4, 1024, True), nn.LeakyReLU(inplace=True), nn.Linear(1024, 1, True))
        self._initialize_weights()

    def _initialize_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                fan_out = m.out_channels * m.kernel_size[0] * m.kernel_size[1]
                nn.init.normal_(m.weight, 0.0, math.sqrt(2.0 / fan_out))
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0.0, 0.01)
            else:
                continue
            if m.bias is not None:
                nn.init.zeros_(m.bias)

    def forward(self, x):
        assert tuple(x.shape[1:]) == (self.input_channels, self.resolution, self.resolution), tuple(x.shape)
        x = run_layers(self.features, x)
        return self.classifier(x.reshape(x.size(0), -1))
