"""``LossNetUnshaded``: training loss on the unshaded G-buffer (mask, normal, depth, AO).

Public surface of ``SuperresolutionNetwork/losses/lossnet_unshaded.py`` (constructor arguments,
``forward(gt, pred, input, prev_input_warped, prev_pred_warped) -> (loss, {key: float})``,
static ``pad``) for the l1 / mse(l2) / temp-l2 terms of the README recipe
``l1:mask:1,l1:ao:1,l1:normal:10,l1:depth:10,temp-l2:color:0.1``:

* spec mini-language ``name:target[:weight]`` (``:30,45-107``); ``('mse','color')`` with weight 0 is
  always evaluated because PSNR is derived from it (``:37-38``);
* a border of ``padding`` pixels of gt / pred / prev is zeroed first (``pad``, ``:171-185`` -- note the
  reference crops both axes with the *height*, so only square inputs are meaningful there; here
  each axis uses its own size, identical for squares);
* normals are re-normalised, the gt mask ``clamp(m/2+1/2, 0, 1)`` gates normal / ao / depth terms
  (``:236-256``); colours come from an internal shader with fov 30, light (0,0,1), white material,
  specular off, strengths from ``opt.lossAmbient / lossDiffuse / lossSpecular / lossAO`` (``:116-126``);
* ``temp-l2`` compares against the warped previous prediction (``:357-388``);
* the downsample-consistency terms ``l2-ds`` / ``l1-ds`` on mask / normal / depth / color (``:63-70``, ``:258-282``): the l2 / l1 loss
  between the upsampled INPUT and the prediction, both resized by 1 / upscale_factor (bilinear: with factor 4 the mean of the centre
  2 x 2 pixels of every 4 x 4 cell), normal and depth gated by the INPUT's mask, the input shaded with AO factor 1 (it has five
  channels) and NOT padded, so the zeroed border of the prediction contributes.  Target ``ao`` raises: the reference's own forward
  cannot run it (``input_ao = None``, ``:225``).  On the GPU two launches forward and one backward in the fused loss's autograd node
  (``ops.loss_unshaded_ds``);
* the adversarial terms ``adv`` / ``gan`` (spatio-temporal, 26 channels), ``tgan`` (temporal, 16) and ``sgan`` (spatial, 13), target
  ``all`` (``:80-105``, ``:313-354``): each owns a discriminator built by ``LossBuilder.gan_loss(opt.discriminator, ...)`` and adds
  ``weight * BCE-with-logits(discriminator(input), 1)`` to the generator's loss; ``train_discriminator`` (``:414-495``) is the
  discriminators' own loss on a ground-truth and a predicted input.  The tensors fed to a discriminator (normalise, shade, pad,
  concatenate) are ``ops.discriminator_input``: one launch each way on the GPU where ``fused`` and its predicate hold, the composition
  of torch operators otherwise; the networks run on ``ops.conv3x3`` / ``ops.conv3x3_s2``.

Parity: the l1 / mse / temp-l2 terms are checked against hand-derived values; the ds terms against values recorded from the reference's
own modules with the one name bound that its ``LossBuilder.downsample_loss`` misses (tests/golden/make_ds_fixtures.py); the adversarial terms, ``train_discriminator`` and the
discriminators against values recorded from the reference's own modules (tests/golden/make_gan_fixtures.py, which supplies an empty
stand-in for the ``torchvision`` import that only the VGG terms use).
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..utils import ScreenSpaceShading


class LossBuilder:
    """Factory of the elementary loss modules ``LossNetUnshaded`` is assembled from (``SuperresolutionNetwork/losses/lossbuilder.py``): the
    terms of the hot-path training recipe (``l1``, ``mse``; README.md:45-64), the downsample-consistency loss (``:343-406``) and the adversarial loss with the reference's two EnhanceNet
    discriminators (``:232-258``, ``:306-331``).  The reference's VGG perceptual / texture losses need a download of VGG19 weights
    (``lossbuilder.py:10,173``): out of scope, they raise; so do the TecoGAN discriminator and the
    Wasserstein form."""

    def __init__(self, device):
        self.device = device

    def mse(self):
        return nn.MSELoss()

    def l1_loss(self):
        return nn.L1Loss()

    def _unsupported(self, what):
        raise NotImplementedError("%s is outside the accelerated hot path (SURVEY.md section 2, row 12)" % what)

    class DownsampleLoss(nn.Module):
        """``lossbuilder.py:343-377``: ``loss`` ('l1' | 'l2', with ``reduction``) between the two arguments resized by
        ``1 / downsample_factor`` (``nn.Upsample``, ``downsample_mode``) -- is the super-resolved image, brought back to the input's
        resolution, the image that was given?  ``gt_low_res``: the first argument already has the low resolution and is taken as it is.
        Bilinear with factor 4 reads the centre 2 x 2 pixels of every 4 x 4 cell (source coordinate 4 d + 1.5) and is their plain mean."""

        def __init__(self, loss, downsample_factor, downsample_mode, gt_low_res, reduction):
            super().__init__()
            self.sample = nn.Upsample(scale_factor=1.0 / downsample_factor, mode=downsample_mode)
            if loss == 'l1':
                self.loss = nn.L1Loss(reduction=reduction)
            elif loss == 'l2':
                self.loss = nn.MSELoss(reduction=reduction)
            else:
                raise ValueError("unknown loss: " + str(loss) + ", expected 'l1' or 'l2'")
            self.gt_low_res = gt_low_res

        def forward(self, gt, pred):
            return self.loss(gt if self.gt_low_res else self.sample(gt), self.sample(pred))

    def downsample_loss(self, loss, downsample_factor, downsample_mode='bilinear', low_res_gt=False, reduction='mean'):
        """``lossbuilder.py:379-406``.  (As shipped the reference names its nested class without the qualifier, ``:404``, and raises
        ``NameError`` here; this is the evident intent.)"""
        return LossBuilder.DownsampleLoss(loss, downsample_factor, downsample_mode, low_res_gt, reduction).to(self.device)

    class AdversarialLoss(nn.Module):
        """``lossbuilder.py:232-258``: the non-saturating GAN loss on logits.  ``forward(x)``: the generator's loss, BCE of the
        discriminator's logits for a prediction against the label TRUE.  ``train_discr``: the discriminator's loss, BCE of its logits for
        the ground-truth input against TRUE plus for the predicted input against FAKE, and the mean sigmoid of both (floats, as the
        reference returns them; detached tensors with ``lazy_values``, so that a step can be enqueued without a stall).  The labels are
        float tensors: the reference's ``torch.full(shape, 1)`` was written when that gave the default float type."""
        TRUE_LABEL = 1
        FAKE_LABEL = 0

        def __init__(self):
            super().__init__()
            self.lazy_values = False

        @staticmethod
        def _bce(logits, label):
            return F.binary_cross_entropy_with_logits(logits, torch.full(logits.shape, float(label), dtype=logits.dtype, device=logits.device))

        def forward(self, x):
            return self._bce(x, LossBuilder.AdversarialLoss.TRUE_LABEL)

        def train_discr(self, gt_input, pred_input, discr):
            gt_logits = discr(gt_input)
            pred_logits = discr(pred_input)
            gt_score = torch.mean(torch.sigmoid(gt_logits)).detach()
            pred_score = torch.mean(torch.sigmoid(pred_logits)).detach()
            if not self.lazy_values:
                gt_score, pred_score = gt_score.item(), pred_score.item()
            loss = self._bce(gt_logits, LossBuilder.AdversarialLoss.TRUE_LABEL) + self._bce(pred_logits, LossBuilder.AdversarialLoss.FAKE_LABEL)
            return loss, gt_score, pred_score

    def build_discriminator(self, model, resolution, input_channels, additional_opt):
        """``lossbuilder.py:306-322``: the discriminator named ``model`` (case-insensitive)."""
        name = str(model).lower()
        if name == 'enhancenetsmall':
            from .enhancenetsmall import EnhanceNetSmallDiscriminator
            return EnhanceNetSmallDiscriminator(resolution, input_channels)
        if name == 'enhancenetlarge':
            from .enhancenetlarge import EnhanceNetLargeDiscriminator
            return EnhanceNetLargeDiscriminator(resolution, input_channels)
        if name == 'tecogan':
            raise NotImplementedError("the tecoGAN discriminator (4x4 convolutions, LeakyReLU slope 0.2) has no kernels in this package; "
                                      "use enhanceNetSmall or enhanceNetLarge")
        raise ValueError('Unsupported discriminator model: %s' % model)

    def gan_loss(self, model, resolution, input_channels, additional_opt):
        """``lossbuilder.py:324-331`` -> (discriminator, AdversarialLoss)."""
        return self.build_discriminator(model, resolution, input_channels, additional_opt), LossBuilder.AdversarialLoss()

    def wgan_loss(self, *a, **k):
        # (the reference's own train_discr for it reads names it never defines, lossbuilder.py:284-296)
        self._unsupported("the Wasserstein adversarial loss")

    def get_style_and_content_loss(self, *a, **k):
        self._unsupported("VGG perceptual/texture loss")


_TARGETS = ('mask', 'normal', 'color', 'ao', 'depth', 'all')


class LossNetUnshaded(nn.Module):
    # forward() accepts the upsampled low-resolution input and its warped predecessor like the reference's; only the adversarial
    # terms read them: train.clip_loss skips producing them for a criterion without a discriminator (an instance with one sets
    # uses_input = True), and so does one with a downsample-consistency term, which reads the upsampled input alone
    # (uses_previous_input = False: the recurrence then neither resizes nor warps input[:, j-1])
    uses_input = False
    uses_previous_input = False

    def __init__(self, device, input_channels, output_channels, high_res, padding, opt):
        super().__init__()
        # the reference returns the per-term values as Python floats (one device synchronisation per term and frame);
        # lazy_values = True returns detached tensors instead, so that a training step can be enqueued without stalls
        self.lazy_values = False
        # GPU tensors: the whole forward is ONE launch of isrLossUnshadedForward (+ a one-workgroup reduction) and the
        # whole backward ONE launch of isrLossUnshadedBackward (csrc/sr_train.hip) instead of ~350 PyTorch launches per
        # frame, the ds terms add two launches forward and one backward inside the same autograd node (ops.loss_unshaded_ds),
        # and each adversarial term's discriminator input is one launch each way (ops.discriminator_input);
        # fused = False keeps the module path below (what the CPU runs, and what the GPU tests compare against)
        self.fused = True
        self._fused_cfg = (None, None)
        self.padding = padding
        self.upsample = opt.upsample
        assert input_channels == 5
        assert output_channels == 6
        self.loss_list = [s.split(':') for s in opt.losses.split(',')]
        builder = LossBuilder(device)
        loss_dict = {'mse': builder.mse()}
        self.weight_dict = {('mse', 'color'): 0.0}
        self.has_discriminator = False
        self.has_style_or_content_loss = False
        self.has_temporal_l2_loss = False
        self.has_downsample_loss = False
        for entry in self.loss_list:
            if len(entry) < 2:
                raise ValueError("illegal format for loss list: " + ':'.join(entry))
            name, target = entry[0], entry[1]
            weight = float(entry[2]) if len(entry) > 2 else 1.0
            if target not in _TARGETS:
                raise ValueError("Unknown target: " + target)
            if name in ('mse', 'l2', 'l2_loss'):
                self.weight_dict[('mse', target)] = weight
            elif name in ('l1', 'l1_loss'):
                loss_dict['l1'] = builder.l1_loss()
                self.weight_dict[('l1', target)] = weight
            elif name in ('tl2', 'temp-l2'):
                loss_dict['temp-l2'] = builder.mse()
                self.weight_dict[('temp-l2', target)] = weight
                self.has_temporal_l2_loss = True
            elif name in ('adv', 'gan', 'tgan', 'sgan'):
                # (:80-105) spatio-temporal: input + previous input + prediction + previous prediction (5 + 5 + 8 + 8); temporal: the two
                # predictions; spatial: input + prediction
                assert target == 'all'
                attr, key, channels = {'adv': ('', 'adv', 26), 'gan': ('', 'adv', 26), 'tgan': ('temp_', 'tgan', 16),
                                       'sgan': ('spatial_', 'sgan', 13)}[name]
                discr, adv = builder.gan_loss(opt.discriminator, high_res, channels, opt)
                setattr(self, attr + 'discriminator', discr)
                setattr(self, attr + 'adv_loss', adv)
                self.weight_dict[(key, target)] = weight
                if key == 'adv':
                    self.discriminator_use_previous_image = True
                    self.discriminator_clip_weights = False
                self.has_discriminator = True
                self.uses_input = True
                self.uses_previous_input = True
            elif name in ('l2-ds', 'l1-ds'):
                # (:63-70) is the prediction, resized to the input's resolution, the input?
                if target == 'ao':
                    raise NotImplementedError("loss '%s:ao': the input has no ambient occlusion channel -- the reference's own forward cannot "
                                              "run this term (it multiplies None, lossnet_unshaded.py:225,272)" % name)
                if target == 'all':
                    raise ValueError("loss '%s' has no target 'all'" % name)
                loss_dict[name] = builder.downsample_loss(name[:2], getattr(opt, 'upscale_factor', 4), 'bilinear')
                self.weight_dict[(name, target)] = weight
                self.has_downsample_loss = True
                self.uses_input = True
            elif name in ('perceptual', 'texture'):
                raise NotImplementedError("loss '%s' is outside the accelerated hot path" % name)
            else:
                raise ValueError('unknown loss %s' % name)
        self.loss_dict = nn.ModuleDict(loss_dict)
        print('Loss weights:', self.weight_dict)

        sh = ScreenSpaceShading(device)
        sh.fov(30)
        sh.ambient_light_color(np.array([opt.lossAmbient] * 3))
        sh.diffuse_light_color(np.array([opt.lossDiffuse] * 3))
        sh.specular_light_color(np.array([getattr(opt, 'lossSpecular', 0.0)] * 3))
        sh.specular_exponent(16)
        sh.enable_specular = False
        sh.light_direction(np.array([0.0, 0.0, 1.0]))
        sh.material_color(np.array([1.0, 1.0, 1.0]))
        sh.ambient_occlusion(opt.lossAO)
        self.shading = sh
        print('LossNet: ambient occlusion strength:', opt.lossAO)

    _DISCRIMINATORS = ('discriminator', 'temp_discriminator', 'spatial_discriminator')

    def discriminators(self):
        """{attribute name: module} of the discriminators this criterion owns (none without an adversarial term)."""
        return {name: getattr(self, name) for name in self._DISCRIMINATORS if hasattr(self, name)}

    def get_discr_parameters(self):
        return [p for d in self.discriminators().values() for p in d.parameters()]

    def discr_eval(self):
        for d in self.discriminators().values():
            d.eval()

    def discr_train(self):
        for d in self.discriminators().values():
            d.train()

    @staticmethod
    def pad(img, border):
        """Overwrites a ``border``-pixel frame of ``img`` with zeros (size unchanged)."""
        return ops.pad_border(img, border)

    def _fusable(self, gt, pred, prev):
        return (self.fused and pred.is_cuda and gt.is_cuda and pred.dtype == torch.float32 and gt.dtype == torch.float32
                and pred.shape[3] % 4 == 0 and 2 * self.padding < min(pred.shape[2], pred.shape[3])
                and not self.shading.enable_specular
                and (prev is None or (prev.is_cuda and prev.dtype == torch.float32 and prev.shape == pred.shape)))

    def _fused_inputs(self, cur, prev, input, prev_input):
        """Whether the discriminators' inputs of these four tensors are assembled by ``ops.discriminator_input``'s kernels (one launch
        per term and direction) instead of operator by operator."""
        return (self.fused and ops.DISCR_INPUT_FUSED and None not in (cur, prev, input, prev_input)
                and ops.discriminator_input_supported(cur, prev, input, prev_input, padding=self.padding, shading=self.shading))

    # (key, attribute prefix, value key, parts of (input, prev_input, cur, prev) that the term's discriminator reads)
    _ADVERSARIAL_TERMS = (('adv', '', 'discr_pred', (True, True, True, True)), ('tgan', 'temp_', 'temp_discr_pred', (False, False, True, True)),
                          ('sgan', 'spatial_', 'spatial_discr_pred', (True, False, True, False)))

    def _fused_term_input(self, parts, input, prev_input, cur, prev, order, cur_raw_normal):
        return ops.discriminator_input(cur, prev if parts[3] else None, input if parts[0] else None, prev_input if parts[1] else None,
                                       padding=self.padding, shading=self.shading, order=order, cur_raw_normal=cur_raw_normal)

    def _forward_fused(self, gt, pred, prev, input=None):
        fused_weights = {k: v for k, v in self.weight_dict.items() if k[0] in ops.LOSS_KINDS}       # (the adversarial terms are added by forward)
        ds_weights = {k: v for k, v in self.weight_dict.items() if k[0] in ops.LOSS_DS_KINDS}
        key = (tuple(self.shading.packed_parameters()), self.shading._ao, bool(self.shading.inverse_ao), self.padding,
               tuple(sorted(fused_weights.items())), tuple(sorted(ds_weights.items())))
        if self._fused_cfg[0] != key:
            self._fused_cfg = (key, ops.loss_unshaded_config(fused_weights, self.padding, self.shading),
                               ops.loss_downsample_config(ds_weights, self.padding, self.shading) if ds_weights else None)
        prev = prev if self.has_temporal_l2_loss else None
        if ds_weights:
            vals = ops.loss_unshaded_ds(gt, pred, prev, input, self._fused_cfg[1], self._fused_cfg[2])
        else:
            vals = ops.loss_unshaded(gt, pred, prev, self._fused_cfg[1])
        host = None if self.lazy_values else vals.detach().tolist()
        values = {}
        for kind in ('mse', 'l1'):
            for target in ('mask', 'normal', 'ao', 'depth', 'color'):
                if (kind, target) in self.weight_dict:
                    t = ops.LOSS_KINDS.index(kind) * 5 + ops.LOSS_TARGETS.index(target)
                    values[(kind, target)] = vals[t].detach() if self.lazy_values else host[t]
        for kind in ops.LOSS_DS_KINDS:
            for target in ops.LOSS_DS_TARGETS:
                if (kind, target) in self.weight_dict:
                    t = 16 + ops.LOSS_DS_KINDS.index(kind) * 4 + ops.LOSS_DS_TARGETS.index(target)
                    values[(kind, target)] = vals[t].detach() if self.lazy_values else host[t]
        for target in ('mask', 'normal', 'ao', 'depth', 'color'):
            if ('temp-l2', target) in self.weight_dict:
                t = 10 + ops.LOSS_TARGETS.index(target)
                values[('temp-l2', target)] = vals[t].detach() if self.lazy_values else host[t]
        return vals[15], values

    def forward(self, gt, pred, input, prev_input_warped, prev_pred_warped):
        B, Cout, Hh, Wh = gt.shape
        assert Cout == 6
        assert gt.shape == pred.shape
        if self.has_downsample_loss and input is None:
            raise ValueError("the downsample-consistency terms need the upsampled input")
        # (a ds term whose operands the ds kernels do not take -- a height or width that is no multiple of 4, an input that needs a
        # gradient -- sends the whole criterion down the module path for this call)
        if self._fusable(gt, pred, prev_pred_warped) and (not self.has_downsample_loss
                                                          or ops.loss_downsample_supported(pred, input, self.padding)):
            # the fused launches compute the l1 / mse / temp-l2 / ds part; the adversarial terms are added to its total
            total, values = self._forward_fused(gt, pred, prev_pred_warped, input)
            if self.has_discriminator:
                if self._fused_inputs(pred, prev_pred_warped, input, prev_input_warped):
                    # the assembly kernel zeroes the border itself and shades: the unpadded prediction goes in
                    adv, adv_values = self._adversarial_terms(pred, None, input, prev_input_warped, prev_pred_warped)
                else:
                    pred_pad = LossNetUnshaded.pad(pred, self.padding)
                    adv, adv_values = self._adversarial_terms(pred_pad, self.shading(pred_pad), input, prev_input_warped,
                                                              LossNetUnshaded.pad(prev_pred_warped, self.padding))
                total = total + adv
                values.update(adv_values)
            return total, values
        gt = LossNetUnshaded.pad(gt, self.padding)
        pred = LossNetUnshaded.pad(pred, self.padding)
        if prev_pred_warped is not None:
            prev_pred_warped = LossNetUnshaded.pad(prev_pred_warped, self.padding)

        norm = ScreenSpaceShading.normalize
        gt_mask, pred_mask = gt[:, 0:1], pred[:, 0:1]
        gate = torch.clamp(gt_mask * 0.5 + 0.5, 0, 1)
        fields = {
            'mask': (gt_mask, pred_mask),
            'normal': (norm(gt[:, 1:4], dim=1) * gate, norm(pred[:, 1:4], dim=1) * gate),
            'ao': (gt[:, 5:6] * gate, pred[:, 5:6] * gate),
            'depth': (gt[:, 4:5] * gate, pred[:, 4:5] * gate),
        }
        gt_color = self.shading(gt)
        pred_color = self.shading(pred)
        fields['color'] = (gt_color, pred_color)

        total = 0.0
        values = {}
        for name in ('mse', 'l1'):
            for target in ('mask', 'normal', 'ao', 'depth', 'color'):
                key = (name, target)
                if key in self.weight_dict:
                    a, b = fields[target]
                    loss = self.loss_dict[name](a, b)
                    values[key] = loss.detach() if self.lazy_values else loss.item()
                    total = total + self.weight_dict[key] * loss

        if self.has_downsample_loss:
            # (:258-282) the upsampled input -- NOT padded, gated by its own mask, five channels: the shader's AO factor is 1 -- against the
            # padded prediction: a border pixel of the prediction contributes its zeroed fields (and the shader of a zero pixel is not 0)
            input_gate = torch.clamp(input[:, 0:1] * 0.5 + 0.5, 0, 1)
            dfields = {
                'mask': lambda: (input[:, 0:1], pred_mask),
                'normal': lambda: (norm(input[:, 1:4], dim=1) * input_gate, norm(pred[:, 1:4], dim=1) * input_gate),
                'depth': lambda: (input[:, 4:5] * input_gate, pred[:, 4:5] * input_gate),
                'color': lambda: (self.shading(input), pred_color),
            }
            for name in ('l2-ds', 'l1-ds'):
                for target in ('mask', 'normal', 'depth', 'color'):
                    key = (name, target)
                    if key in self.weight_dict:
                        a, b = dfields[target]()
                        loss = self.loss_dict[name](a, b)
                        values[key] = loss.detach() if self.lazy_values else loss.item()
                        total = total + self.weight_dict[key] * loss

        if self.has_discriminator:
            adv, adv_values = self._adversarial_terms(pred, pred_color, input, prev_input_warped, prev_pred_warped)
            total = total + adv
            values.update(adv_values)

        if self.has_temporal_l2_loss:
            crit = self.loss_dict['temp-l2']
            prev = prev_pred_warped
            tfields = {
                'mask': lambda: (pred_mask, prev[:, 0:1]),
                'normal': lambda: (fields['normal'][1], norm(prev[:, 1:4], dim=1) * gate),
                'ao': lambda: (fields['ao'][1], prev[:, 5:6] * gate),
                'depth': lambda: (fields['depth'][1], prev[:, 4:5] * gate),
                'color': lambda: (pred_color, self.shading(prev)),
            }
            for target in ('mask', 'normal', 'ao', 'depth', 'color'):
                key = ('temp-l2', target)
                if key in self.weight_dict:
                    a, b = tfields[target]()
                    loss = crit(a, b)
                    values[key] = loss.detach() if self.lazy_values else loss.item()
                    total = total + self.weight_dict[key] * loss
        return total, values

    def _adversarial_terms(self, pred, pred_color, input, prev_input_warped, prev_pred_warped):
        """The generator's adversarial terms (``:313-354``) -> (weighted sum, {'discr_pred' | 'temp_discr_pred' | 'spatial_discr_pred': value}).
        ``pred`` and ``prev_pred_warped`` arrive with their border already zeroed and ``pred_color`` is the shading of that ``pred``: the
        reference pads, then normalises and shades, then pads AGAIN (``:205-208``, ``:333-336``) -- a zeroed normal shades to the ambient
        term, which the second padding removes.  ``pred_color`` None: the fused branch of ``forward``, ``pred`` and
        ``prev_pred_warped`` arrive UNPADDED and each term's input is one launch of ``ops.discriminator_input``."""
        if input is None or prev_input_warped is None or prev_pred_warped is None:
            raise ValueError("the adversarial terms need the upsampled input, the warped previous input and the warped previous prediction")
        if pred_color is None:
            total, values = 0.0, {}
            for key, attr, value_key, parts in self._ADVERSARIAL_TERMS:
                if (key, 'all') in self.weight_dict:
                    # generator side: mask, normal, COLOUR, ao, the prediction shaded from its unnormalised normal (:315-319, :322-331)
                    x = self._fused_term_input(parts, input, prev_input_warped, pred, prev_pred_warped, order=0, cur_raw_normal=True)
                    loss = getattr(self, attr + 'adv_loss')(getattr(self, attr + 'discriminator')(x))
                    values[value_key] = loss.detach() if self.lazy_values else loss.item()
                    total = total + self.weight_dict[(key, 'all')] * loss
            return total, values
        # generator side: mask, normal, COLOUR, ao (:315-319, :322-331) -- train_discriminator below orders ao before colour
        part = dict(padding=self.padding, shading=self.shading, order=0)
        tensors = (LossNetUnshaded.pad(input, self.padding), LossNetUnshaded.pad(prev_input_warped, self.padding),
                   ops.discriminator_part(pred, raw_normal=True, color=pred_color, **part), ops.discriminator_part(prev_pred_warped, **part))
        total, values = 0.0, {}
        for key, attr, value_key, parts in self._ADVERSARIAL_TERMS:
            if (key, 'all') in self.weight_dict:
                x = torch.cat([t for t, used in zip(tensors, parts) if used], dim=1)
                loss = getattr(self, attr + 'adv_loss')(getattr(self, attr + 'discriminator')(x))
                values[value_key] = loss.detach() if self.lazy_values else loss.item()
                total = total + self.weight_dict[(key, 'all')] * loss
        return total, values

    def train_discriminator(self, input, gt_high, previous_input, gt_prev_warped, pred_high, pred_prev_warped):
        """The discriminators' loss for one frame (``:414-495``), everything at high resolution: ``input`` and ``previous_input``
        [B, 5, H, W] (mask, normal, depth), the other four [B, 6, H, W] -> (loss, gt score, pred score), each the weighted sum over the
        adversarial terms of ``AdversarialLoss.train_discr`` on a ground-truth and a predicted input."""
        assert self.has_discriminator
        # discriminator side: mask, normal, AO, colour, shaded from the normalised normal (:436) -- the generator side above orders colour
        # before ao
        if (self._fused_inputs(gt_high, gt_prev_warped, input, previous_input)
                and self._fused_inputs(pred_high, pred_prev_warped, input, previous_input)):
            def term_inputs(parts):
                return tuple(self._fused_term_input(parts, input, previous_input, cur, prev, order=1, cur_raw_normal=False)
                             for cur, prev in ((gt_high, gt_prev_warped), (pred_high, pred_prev_warped)))
        else:
            part = dict(padding=self.padding, shading=self.shading, order=1)
            shared = (LossNetUnshaded.pad(input, self.padding), LossNetUnshaded.pad(previous_input, self.padding))
            sides = tuple(shared + (ops.discriminator_part(cur, **part), ops.discriminator_part(prev, **part))
                          for cur, prev in ((gt_high, gt_prev_warped), (pred_high, pred_prev_warped)))

            def term_inputs(parts):
                return tuple(torch.cat([t for t, used in zip(side, parts) if used], dim=1) for side in sides)
        discr_loss = gt_score = pred_score = 0
        for key, attr, _, parts in self._ADVERSARIAL_TERMS:
            if (key, 'all') in self.weight_dict:
                adv = getattr(self, attr + 'adv_loss')
                adv.lazy_values = self.lazy_values
                gt_input, pred_input = term_inputs(parts)
                loss0, gt0, pred0 = adv.train_discr(gt_input, pred_input, getattr(self, attr + 'discriminator'))
                w = self.weight_dict[(key, 'all')]
                discr_loss, gt_score, pred_score = discr_loss + w * loss0, gt_score + w * gt0, pred_score + w * pred0
        return discr_loss, gt_score, pred_score
