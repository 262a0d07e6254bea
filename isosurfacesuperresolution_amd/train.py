"""Training step of the unshaded temporal network, and its data-parallel form.

Restates ``trainNormal`` of ``SuperresolutionNetwork/mainVideoUnshaded.py:397-473`` (optimizer and
scheduler of ``:287-300``: Adam(lr 1e-4), ``StepLR(lrStep, 0.5)`` stepped at epoch start; seeds of
``:170-171``):

    for each clip [B, T, ...]:   loss = 0, previous_output = None
      for j in range(T):
        j == 0: previous_warped = initialImage(input[:,0], 6, mode);  previous_warped_loss = target[:,0]
        j  > 0: previous_warped = warp_upscale(previous_output, flow[:,j-1], 4, special_mask=True)
        prediction = model(cat(input[:,j], flatten_high(previous_warped, 4)))
        loss += criterion(target[:,j], prediction, up(input[:,j]), previous_input, previous_warped_loss)
        previous_output = cat(clamp(mask), normalize(normal), clamp(depth), clamp(ao))   # NOT detached
      loss.backward(); optimizer.step()

The reference writes that frame loop out in every trainer, test pass and statistics script.  Here it stands once, as the generator
``clip_recurrence`` (initial image, warp of the fed-back output, ``flatten_high`` + ``cat``, the forward, the upsampled inputs of the
adversarial terms), and the fed-back image once, as ``utils.clamp_prediction``; every loop below is "for frame in clip_recurrence:
call the criterion, accumulate":

    ``clip_loss``                 the loop above (``trainNormal``, and the generator phase of the adversarial mode); may take the
                                  fused ``ops.recurrent_input`` for feedback + warp + cat
    ``discriminator_clip_loss``   the generator under ``no_grad``, ``criterion.train_discriminator`` per frame (``:511-566``)
    ``evaluate``                  ``test(epoch)`` (``:639-726``): no gradients, every term of the criterion averaged
    ``colour_clip_loss``          the colour networks (``mainVideo.py:381-434``: three output channels, starts from zeros, the clamped
                                  prediction is what the criterion sees and what is fed back, a criterion the caller brings);
                                  ``train_step`` and ``GraphedTrainStep`` take it as ``clip_loss=``
    ``stats.run_clip`` / ``stats.run_colour_clip``   the two tables, a clip as a batch of one

``adversarial_step`` / ``fit_adversarial`` restate the reference's second training mode, ``trainAdv_v2`` (``:475-636``), which it
enters as soon as ``--losses`` names an adversarial term (``:296-312``): per batch the discriminators are trained on the generator's
frozen predictions, then the generator against the discriminators.

``GraphedTrainStep`` and ``GraphedAdversarialStep`` are those two steps captured in a HIP graph; how a step is warmed up, captured,
put back and replayed is ``_CapturedStep``'s, once.  ``save_checkpoint`` / ``save_adversarial_checkpoint`` write through one writer.

The reference has nothing distributed.  ``DataParallelTrainer`` adds the
MI355X form: one process per GPU, the global batch split over ranks, identical initial weights
(rank 0 broadcast), and after ``backward`` ONE all-reduce of a single flat 3.64 MB gradient bucket
(911 046 fp32; RCCL over xGMI is latency bound at this size, so per-layer buckets would only add
launches), averaged, then a local Adam step.  Loss terms are batch means, so averaged gradients
equal the single-process gradients of the global batch.
"""
import collections
import contextlib
import os
import warnings

import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import ops
from .models import VideoTools
from .utils import clamp_prediction, initialImage


def backward(loss):
    """``loss.backward()`` with the weight gradients of the HIP convolutions deferred to ONE pass per layer over all
    frames of the clip (``ops.deferred_weight_gradients``) instead of one pass per layer and frame.

    Limitation: a deferred gradient is added to ``param.grad`` when the context exits and does not pass through
    autograd's accumulation, so hooks registered on a convolution weight would not see it -- parameters that carry
    tensor hooks or post-accumulate-grad hooks are detected and keep the ordinary per-frame path
    (``ops._weight_grad_or_defer``).  ``DataParallelTrainer`` reduces ``param.grad`` after this call and is unaffected."""
    with ops.deferred_weight_gradients():
        loss.backward()


Frame = collections.namedtuple("Frame", "j output previous_warped_loss input_high previous_input")


def clip_recurrence(forward, input, flow, channels, target=None, initial_image="zero", upscale=4, disable_temporal=False,
                    special_mask=True, feedback=None, fused=False, upsample=None, previous_input=True):
    """The reference's clip recurrence, stated once (mainVideoUnshaded.py:413-465 and its copies in the discriminator phase, the test
    pass, mainVideo.py:381-434 and the two statistics scripts).  input [B,T,C,h,w], flow [B,T,2,h,w]; for every frame j

        j == 0 or disable_temporal:  previous_warped = initialImage(input[:,0], channels, initial_image)
        otherwise:                   previous_warped = warp_upscale(feedback(output of frame j-1), flow[:,j-1], special_mask)
        output = forward(cat(input[:,j], flatten_high(previous_warped)))

    and yields a ``Frame`` (j, output, previous_warped_loss, input_high, previous_input) for the caller to consume.  ``output`` is whatever
    ``forward`` returns -- the caller decides there whether the model runs under ``no_grad``, through a guard, with a clamp behind it;
    ``feedback`` (identity unless given) makes the image that is warped into the next frame from it, NOT detached.
    ``previous_warped_loss``: target[:,0] where a frame starts from the initial image, ``previous_warped`` elsewhere (None without a
    ``target``).  ``upsample`` (an interpolation mode): the low-resolution inputs the reference hands to its criterion
    (mainVideoUnshaded.py:432-452) -- ``input_high`` = input[:,j] upsampled, ``previous_input`` = input[:,j-1] upsampled and warped
    (input[:,0] upsampled at a start); both None without it; ``previous_input=False`` (a criterion that reads ``input_high`` alone,
    ``LossNetUnshaded.uses_previous_input``) leaves ``Frame.previous_input`` None and enqueues neither its resize nor its warp.  ``fused``: where ``ops.recurrent_input`` supports the operands, feedback
    (it is ``clamp_prediction`` there), warp, space-to-depth and cat are ONE kernel on the raw output."""
    size = (input.shape[3] * upscale, input.shape[4] * upscale)
    kw = dict(mode=upsample, **({"align_corners": False} if upsample in ("bilinear", "bicubic") else {}))
    output = input_high = None
    want_previous, previous_input = previous_input, None
    for j in range(input.shape[1]):
        single_input = None
        if j == 0 or disable_temporal:
            previous_warped = initialImage(input[:, 0], channels, initial_image, False, upscale)
            previous_warped_loss = target[:, 0] if target is not None else None
            if upsample and want_previous:
                previous_input = F.interpolate(input[:, 0], size=size, **kw)
        else:
            if fused and ops.recurrent_input_supported(output, input[:, j], flow[:, j - 1], upscale):
                single_input, previous_warped = ops.recurrent_input(output, input[:, j], flow[:, j - 1])
            else:
                previous_output = output if feedback is None else feedback(output)
                previous_warped = VideoTools.warp_upscale(previous_output, flow[:, j - 1], upscale, special_mask=special_mask)
            previous_warped_loss = previous_warped
            if upsample and want_previous:
                previous_input = VideoTools.warp_upscale(F.interpolate(input[:, j - 1], size=size, **kw), flow[:, j - 1], upscale,
                                                         special_mask=True)
        if single_input is None:
            single_input = torch.cat((input[:, j], VideoTools.flatten_high(previous_warped, upscale)), dim=1)
        output = forward(single_input)
        if upsample:
            input_high = F.interpolate(input[:, j], size=size, **kw)
        yield Frame(j, output, previous_warped_loss, input_high, previous_input)


@contextlib.contextmanager
def lazy_values(criterion):
    """``criterion.lazy_values = True`` for the block -- the criterion returns its terms as detached tensors, no read-back -- and back to
    what it was however the block ends.  A criterion without the attribute (the colour trainers' callables) is left alone."""
    before = getattr(criterion, 'lazy_values', None)
    if before is not None:
        criterion.lazy_values = True
    try:
        yield
    finally:
        if before is not None:
            criterion.lazy_values = before


def _refresh_split_images(model, target):
    if ops.TRAIN_SPLIT and not ops.TRAIN_BF16 and target.is_cuda and torch.is_grad_enabled():
        # every weight changed in the last optimizer step: refresh all split-kernel weight images in two launches
        ops.prepare_split_many([m.weight for m in model.modules()
                                if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3) and m.out_channels > 8 and m.in_channels > 8])


def clip_loss(model, criterion, input, flow, target, initial_image="zero", upscale=4, upsample="bilinear",
              disable_temporal=False, fused_recurrence=True):
    """input [B,T,5,h,w], flow [B,T,2,h,w], target [B,T,6,4h,4w] -> (loss tensor, sum of the per-frame losses).
    The reference reads every frame's loss back with ``.item()`` (mainVideoUnshaded.py:454); here the sum is accumulated
    on the device and read back ONCE after the last frame, so the whole clip is enqueued without a stall."""
    _refresh_split_images(model, target)
    # only LossNetUnshaded's adversarial and downsample-consistency terms read the upsampled inputs, so a criterion without them
    # says so (uses_input = False) and is not fed; the warped previous input is the adversarial terms' alone (uses_previous_input)
    feed_inputs = getattr(criterion, 'uses_input', True)
    loss, loss_sum = 0, None
    with lazy_values(criterion):
        for f in clip_recurrence(lambda x: model(x)[0], input, flow, target.shape[2], target, initial_image, upscale, disable_temporal,
                                 feedback=clamp_prediction, fused=fused_recurrence, upsample=upsample if feed_inputs else None,
                                 previous_input=getattr(criterion, 'uses_previous_input', True)):
            loss0, _ = criterion(target[:, f.j], f.output, f.input_high, f.previous_input, f.previous_warped_loss)
            loss = loss + loss0
            loss_sum = loss0.detach() if loss_sum is None else loss_sum + loss0.detach()
    return loss, loss_sum


def colour_clip_loss(model, criterion, input, flow, target, upscale=4, disable_temporal=False):
    """The clip recurrence of the reference's colour trainer (``SuperresolutionNetwork/mainVideo.py:381-434``, ``deferredShading``) for a
    three-channel network such as ``models.RCAN``: input [B,T,C,h,w], flow [B,T,2,h,w], target [B,T,3,4h,4w] -> (loss tensor, sum of
    the per-frame losses), as ``clip_loss`` without a host read-back.

        j == 0 (or disable_temporal): previous_warped = zeros [B,3,4h,4w];  previous_warped_loss = target[:,0]          (:386, :395)
        j  > 0: previous_warped = previous_warped_loss = warp_upscale(previous_output, flow[:,j-1], 4)                  (:407-408)
        prediction = clamp(model(cat(input[:,j], flatten_high(previous_warped, 4)))[0], 0, 1)                           (:409-416)
        loss += criterion(target[:,j], prediction, input[:,j], previous_warped_loss)[0]                                 (:418-422)
        previous_output = prediction                                    # NOT detached: gradients flow through time     (:434)

    ``criterion``: any callable with the signature of the reference's ``LossNet.forward`` -> (loss, values).  The reference's own
    call of it is commented out in favour of two hard-wired MSE terms (:424-430), and ``losses.LossNet`` (VGG and GAN terms) is not
    part of this package: the caller brings the criterion."""
    _refresh_split_images(model, target)
    loss, loss_sum = 0, None
    for f in clip_recurrence(lambda x: torch.clamp(model(x)[0], 0, 1), input, flow, target.shape[2], target, "zero", upscale,
                             disable_temporal, special_mask=False):
        loss0, _ = criterion(target[:, f.j], f.output, input[:, f.j], f.previous_warped_loss)
        loss = loss + loss0
        loss_sum = loss0.detach() if loss_sum is None else loss_sum + loss0.detach()
    return loss, loss_sum


def make_optimizer(model, lr=1e-4, lr_step=500, lr_gamma=0.5, capturable=False, tensor_lr=False, flat=False):
    """Adam + StepLR of mainVideoUnshaded.py:287-300.  ``tensor_lr``: the learning rate lives in a device tensor, so that
    a scheduler step is seen by an optimizer step captured in a HIP graph (needs ``capturable``).  ``flat``: ``FlatAdam`` -- the
    same update over one flat buffer in one launch (parameters and gradients become views of it)."""
    params = list(model.parameters())
    if flat:
        opt = FlatAdam(params, lr=lr, tensor_lr=tensor_lr)
        return opt, torch.optim.lr_scheduler.StepLR(opt, lr_step, lr_gamma)
    if tensor_lr:
        lr = torch.tensor(float(lr), dtype=torch.float32, device=params[0].device)
    opt = torch.optim.Adam(params, lr=lr, capturable=capturable)
    sched = torch.optim.lr_scheduler.StepLR(opt, lr_step, lr_gamma)
    return opt, sched


class FlatAdam(torch.optim.Optimizer):
    """``torch.optim.Adam`` (the reference's optimizer, mainVideoUnshaded.py:287-289: lr 1e-4, betas (0.9, 0.999), eps 1e-8, no
    weight decay) over ONE flat buffer: every parameter of the model becomes a view of ``self.flat`` and every gradient a view of
    ``self.bucket``, so a step is one launch (``isrAdamFlatStep``) instead of ~100 per-tensor launches, zeroing the gradients one
    ``zero_``, and the data-parallel exchange one all-reduce of ``self.bucket`` (``DataParallelTrainer`` adopts it).  The step
    counter and (optionally) the learning rate live on the device, so a HIP graph of the step replays correctly.

    Build it AFTER ``model.to(device)`` (moving the model afterwards detaches the views: call ``rebind()``).  A step writes the
    parameters' memory without advancing ``Parameter._version``: it declares the cached kernel-layout weight images stale itself.

    State: the moments and the step counter live in ``self.state[self.flat]`` under torch.optim.Adam's keys (``step``, ``exp_avg``,
    ``exp_avg_sq``), so ``state_dict()`` / ``load_state_dict()`` and pickling the optimizer object -- what the reference's
    checkpoints do (mainVideoUnshaded.py:799-811) -- carry them; the member parameters travel with the pickle and are re-pointed
    at the flat buffers when it is loaded (``__setstate__`` -> ``rebind``).  ``load_state_dict`` copies INTO the existing state
    tensors, so a HIP graph captured before it keeps updating the live ones."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, tensor_lr=False):
        params = [p for p in params if p.requires_grad]
        dev = params[0].device
        self.members = params
        self.flat = self.bucket = None
        flat = self._bind()
        if tensor_lr and not torch.is_tensor(lr):
            lr = torch.tensor(float(lr), dtype=torch.float32, device=dev)
        super().__init__([flat], dict(lr=lr, betas=betas, eps=eps, capturable=True))
        self.state[flat] = dict(step=torch.zeros(1, dtype=torch.float32, device=dev), exp_avg=torch.zeros_like(flat.data),
                                exp_avg_sq=torch.zeros_like(flat.data))

    def _bind(self):
        """(Re)build the flat parameter / gradient buffers from the members' current values and point the members at them."""
        params = self.members
        n = sum(p.numel() for p in params)
        dev, dt = params[0].device, params[0].dtype
        flat = torch.empty(n, dtype=dt, device=dev)
        bucket = torch.zeros(n, dtype=dt, device=dev)
        off = 0
        with torch.no_grad():
            for p in params:
                k = p.numel()
                flat[off:off + k].copy_(p.detach().reshape(-1))
                p.data = flat[off:off + k].view_as(p)
                p.grad = bucket[off:off + k].view_as(p)
                off += k
        self.flat = torch.nn.Parameter(flat)
        self.flat.grad = bucket
        self.bucket = bucket
        return self.flat

    # the moments under their old attribute names (kernel launch, tests)
    exp_avg = property(lambda self: self.state[self.flat]['exp_avg'])
    exp_avg_sq = property(lambda self: self.state[self.flat]['exp_avg_sq'])
    steps = property(lambda self: self.state[self.flat]['step'])

    def views_intact(self):
        if self.flat is None or self.bucket is None or self.flat.grad is not self.bucket:
            return False
        base, pbase, esz, off = self.bucket.data_ptr(), self.flat.data_ptr(), self.bucket.element_size(), 0
        for p in self.members:
            if p.grad is None or p.grad.data_ptr() != base + off * esz or p.data_ptr() != pbase + off * esz or p.device != self.flat.device:
                return False
            off += p.numel()
        return True

    def rebind(self):
        """After the members moved (``model.to(device)``) or the optimizer was unpickled: make parameters and gradients views of
        the flat buffers again, keeping the parameters' CURRENT values and the optimizer's moments / step count / learning rate."""
        if self.views_intact():
            return self
        old = self.flat
        st = self.state.pop(old) if old is not None and old in self.state else None
        flat = self._bind()
        self.param_groups[0]['params'] = [flat]
        if st is None:
            st = dict(step=torch.zeros(1), exp_avg=torch.zeros(flat.numel()), exp_avg_sq=torch.zeros(flat.numel()))
        self.state[flat] = {k: (v.to(device=flat.device, dtype=torch.float32 if k == 'step' else flat.dtype) if torch.is_tensor(v) else v)
                            for k, v in st.items()}
        g = self.param_groups[0]
        if torch.is_tensor(g['lr']) and g['lr'].device != flat.device:
            g['lr'] = g['lr'].to(flat.device)
        return self

    def __getstate__(self):
        st = dict(super().__getstate__())
        st['members'] = self.members
        return st

    def __setstate__(self, state):
        members = state.pop('members', None) if isinstance(state, dict) else None
        super().__setstate__(state)
        if members is not None:                    # unpickled (load_state_dict comes through here too, without members)
            self.members = members
            self.flat = self.param_groups[0]['params'][0]
            self.bucket = None                     # gradients are not pickled
            self.rebind()

    def load_state_dict(self, state_dict):
        live = self.state[self.flat]
        lr_live = self.param_groups[0]['lr']
        super().load_state_dict(state_dict)
        loaded = self.state[self.flat]
        with torch.no_grad():
            for k in ('step', 'exp_avg', 'exp_avg_sq'):
                live[k].copy_(loaded[k].reshape(live[k].shape))
        self.state[self.flat] = live
        if torch.is_tensor(lr_live):               # a captured step reads THIS tensor
            lr_live.fill_(float(self.param_groups[0]['lr']))
            self.param_groups[0]['lr'] = lr_live

    def zero_grad(self, set_to_none=False):
        self.bucket.zero_()

    def check_views(self):
        if not self.views_intact():
            raise RuntimeError("FlatAdam: a parameter or its .grad is no longer a view of the flat buffers "
                               "(model.to() after construction -- call rebind() -- or an optimizer.zero_grad(set_to_none=True) elsewhere)")

    @torch.no_grad()
    def step(self, closure=None):
        g = self.param_groups[0]
        ops.adam_flat_step(self.flat.data, self.bucket, self.exp_avg, self.exp_avg_sq, self.steps, g['lr'], g['betas'][0], g['betas'][1], g['eps'])
        ops.invalidate_weight_images()


def step_scheduler(optimizer, scheduler):
    """``scheduler.step()`` at the START of an epoch, as the reference does (mainVideoUnshaded.py:399; torch >= 1.1 warns
    about the order, the schedule is the reference's).  A learning rate kept in a device tensor is updated IN PLACE:
    a captured optimizer step reads that very tensor."""
    before = [g['lr'] for g in optimizer.param_groups]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        scheduler.step()
    for g, old in zip(optimizer.param_groups, before):
        if isinstance(old, torch.Tensor) and g['lr'] is not old:
            old.fill_(float(g['lr']))
            g['lr'] = old
    return float(optimizer.param_groups[0]['lr'])


def train_step(model, criterion, optimizer, batch, clip_loss=None, **kw):
    """One optimisation step on a clip batch (single process).  ``clip_loss``: the clip's recurrence -- this module's ``clip_loss``
    (the unshaded networks) unless given, ``colour_clip_loss`` for a colour network; ``kw`` goes to it."""
    input, flow, target = batch
    optimizer.zero_grad()          # (FlatAdam: one zero_ of its flat gradient buffer, the views stay)
    loss, loss_sum = (clip_loss or globals()['clip_loss'])(model, criterion, input, flow, target, **kw)
    backward(loss)
    optimizer.step()
    return float(loss_sum.item()) / target.shape[1]


def make_adversarial_optimizers(model, criterion, lr=1e-4, lr_step=500, lr_gamma=0.5, capturable=False):
    """The two optimizers of mainVideoUnshaded.py:303-312: Adam(lr) on the generator, Adam(lr * 0.5) on the discriminators' trainable
    parameters, StepLR(lr_step, lr_gamma) on both -> (gen_optimizer, discr_optimizer, gen_scheduler, discr_scheduler).
    ``capturable``: both Adams keep their step counts on the device, as ``GraphedAdversarialStep`` needs them."""
    discr_params = [p for p in criterion.get_discr_parameters() if p.requires_grad]
    if not discr_params:
        raise ValueError("make_adversarial_optimizers: the criterion has no discriminator (no adv / gan / tgan / sgan term in its losses)")
    gen_optimizer = torch.optim.Adam(list(model.parameters()), lr=lr, capturable=capturable)
    discr_optimizer = torch.optim.Adam(discr_params, lr=lr * 0.5, capturable=capturable)
    return (gen_optimizer, discr_optimizer, torch.optim.lr_scheduler.StepLR(gen_optimizer, lr_step, lr_gamma),
            torch.optim.lr_scheduler.StepLR(discr_optimizer, lr_step, lr_gamma))


def discriminator_clip_loss(model, criterion, input, flow, target, initial_image="zero", upscale=4, upsample="bilinear",
                            disable_temporal=False):
    """The discriminator phase's loop over the frames of a clip (mainVideoUnshaded.py:511-566): the generator runs without gradients,
    ``criterion.train_discriminator`` compares each frame's prediction with the ground truth -> (loss tensor, sum of the gt scores, sum
    of the pred scores; device tensors, nothing is read back)."""
    loss, gt_sum, pred_sum = 0, 0, 0
    with lazy_values(criterion):
        for f in clip_recurrence(torch.no_grad()(lambda x: model(x)[0]), input, flow, target.shape[2], target, initial_image, upscale,
                                 disable_temporal, feedback=clamp_prediction, upsample=upsample):
            # at j = 0 this is frame -1 of the clip, the LAST one, warped by flow[:, -1] (mainVideoUnshaded.py:543-547 index with j - 1)
            gt_prev_warped = VideoTools.warp_upscale(target[:, f.j - 1], flow[:, f.j - 1], upscale, special_mask=True)
            loss0, gt_score, pred_score = criterion.train_discriminator(f.input_high, target[:, f.j], f.previous_input, gt_prev_warped,
                                                                        f.output, f.previous_warped_loss)
            loss, gt_sum, pred_sum = loss + loss0, gt_sum + gt_score, pred_sum + pred_score
    return loss, gt_sum, pred_sum


def adversarial_step(model, criterion, gen_optimizer, discr_optimizer, batch, disc_steps=2, **kw):
    """The body of ``trainAdv_v2`` for one batch (mainVideoUnshaded.py:506-624) -> (discr_loss, gen_loss, gt_score, pred_score): the
    clip's loss of the LAST discriminator step and of the LAST generator step, and the discriminators' scores summed over every
    discriminator step and frame, which is what the reference adds to its epoch totals (:567, :562-563, :621).

    Discriminator phase, ``disc_steps`` times: the generator under ``no_grad``, ``discriminator_clip_loss``, one step of
    ``discr_optimizer``.  Generator phase, ALSO ``disc_steps`` times (the reference's loop reads ``disc_steps``, not its
    ``advGenMaxSteps``, :572): ``clip_loss`` with the adversarial terms, one step of ``gen_optimizer``.  There the discriminators'
    parameters are switched to ``requires_grad_(False)`` and back: the reference computes their gradients and zeroes them unused
    (:508-509, :573-574), so every parameter ends the same.  Both phases go through ``backward`` (deferred weight gradients);
    ``kw`` goes to the two clip loops (initial_image, upscale, upsample, disable_temporal)."""
    return tuple(float(v) for v in _adversarial_step_tensors(model, criterion, gen_optimizer, discr_optimizer, batch, disc_steps, **kw))   # (the step's read-back)


def _adversarial_step_tensors(model, criterion, gen_optimizer, discr_optimizer, batch, disc_steps, **kw):
    """``adversarial_step`` without its read-back: the four results as they come off the device (tensors), so that the same body can be
    enqueued eagerly or captured (``GraphedAdversarialStep``)."""
    input, flow, target = batch
    dkw = {k: v for k, v in kw.items() if k != "fused_recurrence"}
    discr_loss = gen_loss = None
    gt_score = pred_score = 0
    for _ in range(disc_steps):
        discr_optimizer.zero_grad()
        gen_optimizer.zero_grad()
        loss, gt_sum, pred_sum = discriminator_clip_loss(model, criterion, input, flow, target, **dkw)
        backward(loss)
        discr_optimizer.step()
        discr_loss, gt_score, pred_score = loss.detach(), gt_score + gt_sum, pred_score + pred_sum
    discr_params = [p for p in criterion.get_discr_parameters() if p.requires_grad]
    for p in discr_params:
        p.requires_grad_(False)
    try:
        for _ in range(disc_steps):
            discr_optimizer.zero_grad()
            gen_optimizer.zero_grad()
            loss, _ = clip_loss(model, criterion, input, flow, target, **kw)
            backward(loss)
            gen_optimizer.step()
            gen_loss = loss.detach()
    finally:
        for p in discr_params:
            p.requires_grad_(True)
    return discr_loss, gen_loss, gt_score, pred_score


DISCRIMINATOR_KEYS = ('discriminator', 'temp_discriminator', 'spatial_discriminator')


def save_adversarial_checkpoint(modeldir, epoch, model, parameters, criterion, gen_optimizer, discr_optimizer, gen_scheduler, discr_scheduler):
    """``checkpoint(epoch)`` of mainVideoUnshaded.py:799-811 in its adversarial branch: ``save_checkpoint``'s 'epoch', 'model' and
    'parameters', the two optimizer and the two scheduler objects, and each discriminator's ``state_dict`` under its attribute name --
    ``--pretrainedDiscr`` and the reference's restore read ``checkpoint['discriminator']`` (:326, :367).  The whole criterion object of
    :809 is NOT written: the reference never reads it back, and it would need new names in the restricted unpickler."""
    return _write_checkpoint(modeldir, epoch, model, parameters, gen_optimizer=gen_optimizer, discr_optimizer=discr_optimizer,
                             gen_scheduler=gen_scheduler, discr_scheduler=discr_scheduler,
                             **{name: d.state_dict() for name, d in criterion.discriminators().items()})


def fit_adversarial(model, criterion, train_loader, test_loader, modeldir, n_epochs, parameters, device=None, lr=1e-4, lr_step=500,
                    lr_gamma=0.5, disc_steps=2, disc_initial_steps=None, restore=False, restore_epoch=-1, log=print, **kw):
    """The epoch loop of mainVideoUnshaded.py:827-835 for a criterion with adversarial terms:

        for epoch in range(start, n_epochs + 1):  trainAdv_v2(epoch); test(epoch); checkpoint(epoch)

    ``trainAdv_v2`` (:475-636) = both schedulers stepped at the epoch's start, then ``adversarial_step`` per batch with
    ``disc_initial_steps`` discriminator steps in epoch 1 if given, ``disc_steps`` otherwise (``--advDiscrInitialSteps``,
    ``--advDiscrMaxSteps``, :487).  ``restore``: model from the checkpoint, the discriminators' weights loaded into ``criterion``, fresh
    optimizers and schedulers over the LIVE parameters with the checkpointed state loaded into them (the reference takes the pickled
    optimizer objects, :367-371, whose discriminator parameters are copies nothing else uses).  Returns (model, history) -- per epoch
    the four means of ``trainAdv_v2`` (:626-629: sums over batches / (batches x frames)), the learning rates, ``evaluate``'s dict and
    the checkpoint path.  The steps run eagerly (``GraphedAdversarialStep`` is the captured form of one step, for a loop with fixed batch
    shapes).  The loaders are any iterables of (input, flow, target) batches; ``dataset_video.DeviceBatchLoader`` is the fast path (the
    clips resident on the device, a batch one gather launch: ``.to(device)`` below is then a no-op)."""
    if device is None:
        device = next(model.parameters()).device
    start = 1
    ckpt = None
    if restore:
        ckpt, start = load_checkpoint(modeldir, restore_epoch, device)
        model = ckpt['model']
        for name, d in criterion.discriminators().items():
            d.load_state_dict(ckpt[name])
        log("Restore training from %s and epoch %d" % (modeldir, start))
    model = model.to(device)
    criterion.to(device)
    gen_optimizer, discr_optimizer, gen_scheduler, discr_scheduler = make_adversarial_optimizers(model, criterion, lr, lr_step, lr_gamma)
    if ckpt is not None:
        for live, key in ((gen_optimizer, 'gen_optimizer'), (discr_optimizer, 'discr_optimizer'), (gen_scheduler, 'gen_scheduler'),
                          (discr_scheduler, 'discr_scheduler')):
            live.load_state_dict(ckpt[key].state_dict())
    eval_kw = {k: v for k, v in kw.items() if k in ("initial_image", "upscale", "upsample", "disable_temporal")}
    history = []
    for epoch in range(start, n_epochs + 1):
        lr_discr = step_scheduler(discr_optimizer, discr_scheduler)
        lr_gen = step_scheduler(gen_optimizer, gen_scheduler)
        steps = disc_initial_steps if (disc_initial_steps is not None and epoch == 1) else disc_steps
        model.train()
        criterion.discr_train()
        totals, frames = [0.0, 0.0, 0.0, 0.0], 0
        for batch in train_loader:
            batch = tuple(t.to(device, non_blocking=True) for t in batch)
            totals = [a + b for a, b in zip(totals, adversarial_step(model, criterion, gen_optimizer, discr_optimizer, batch, steps, **kw))]
            frames += batch[2].shape[1]
        means = [t / max(1, frames) for t in totals]
        log("===> Epoch {} Complete: discr {:.4f}, gen {:.4f}, gt score {:.4f}, pred score {:.4f}".format(epoch, *means))
        test = evaluate(model, criterion, test_loader, device, **eval_kw) if test_loader is not None else {}
        path = save_adversarial_checkpoint(modeldir, epoch, model, parameters, criterion, gen_optimizer, discr_optimizer, gen_scheduler,
                                           discr_scheduler)
        log("Checkpoint saved to {}".format(path))
        history.append({'epoch': epoch, 'discr_loss': means[0], 'gen_loss': means[1], 'gt_score': means[2], 'pred_score': means[3],
                        'lr_gen': lr_gen, 'lr_discr': lr_discr, 'test': test, 'checkpoint': path})
    return model, history


def _optimizer_state_tensors(optimizer):
    for group in optimizer.param_groups:
        for p in group['params']:
            st = optimizer.state.get(p)
            if st:
                for k, v in st.items():
                    if torch.is_tensor(v):
                        yield (id(p), k), v


def _snapshot_training_state(model, optimizer):
    """Copies of everything an optimisation step changes: the model's parameters and buffers, the optimizer's state tensors."""
    return ({k: v.detach().clone() for k, v in model.state_dict().items()},
            {key: v.detach().clone() for key, v in _optimizer_state_tensors(optimizer)})


@torch.no_grad()
def _restore_training_state(model, optimizer, snapshot):
    """Put model and optimizer back IN PLACE (tensors keep their addresses); optimizer state that did not exist at the
    snapshot (a fresh optimizer creates it in its first step) is zeroed, which is what a first step starts from."""
    weights, opt = snapshot
    for k, v in model.state_dict().items():
        v.copy_(weights[k])
    for key, v in _optimizer_state_tensors(optimizer):
        if key in opt:
            v.copy_(opt[key])
        else:
            v.zero_()


class _CapturedStep:
    """The recipe of a training step captured ONCE in a HIP graph and replayed; a subclass brings ``_eager()`` -- the step on
    ``self.static``, returning device tensors -- and ``zero_grad()``.

    ``_capture``: static batch buffers; ``warmup`` REAL steps on the example batch on a side stream (PyTorch's capture recipe: they
    create the optimizers' state tensors and every cached buffer the capture must find in place); the capture; then every
    (module, optimizer) pair put back to where it was -- in place, the graph holds these very tensors -- because the reference takes one
    step per batch (mainVideoUnshaded.py:397-473).  Before the capture every cached kernel-layout weight image is declared stale: an
    image found valid there -- after an eager forward of the same model with no step since, or of weights that the step's first phase
    leaves alone -- would be taken from the cache with no refresh recorded, and every replay would read that old image.  Stale, each
    weight's first use records its refresh, so the graph rebuilds its own image buffers at the start of every replay.

    A replay changes the weights WITHOUT advancing ``Parameter._version`` (the captured optimizer kernels write the parameters'
    memory directly), so every replay declares the cached images stale again (``ops.invalidate_weight_images``): inference or an
    eager step after a replay re-prepares them from the current weights."""

    def _capture(self, example_batch, pairs, warmup):
        self.static = tuple(torch.empty_like(t) for t in example_batch)
        for dst, src in zip(self.static, example_batch):
            dst.copy_(src)
        before = [_snapshot_training_state(module, optimizer) for module, optimizer in pairs] if warmup > 0 else None
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self._eager()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        self.zero_grad()
        ops.invalidate_weight_images()
        with ops.graph_capture(self.graph):
            captured = self._eager()
        if before is not None:
            for (module, optimizer), snapshot in zip(pairs, before):
                _restore_training_state(module, optimizer, snapshot)
        self.zero_grad()
        ops.invalidate_weight_images()
        return captured

    def _replay(self, batch):
        for dst, src in zip(self.static, batch):
            dst.copy_(src, non_blocking=True)
        self.graph.replay()
        ops.invalidate_weight_images()


class GraphedTrainStep(_CapturedStep):
    """The whole optimisation step (T frames forward with the recurrence, backward through time, Adam) captured ONCE in
    a HIP graph and replayed: at the per-GPU batch of BASELINE config #3 (2 clips) a step is ~1500 small launches and the
    eager loop is bound by Python, not by the GPU.  Needs a GPU, fixed batch shapes, an optimizer created with
    ``capturable=True`` and (as everywhere in this package) no host read-back inside the step; the loss of each step is
    returned as a device tensor.  ``all_reduce`` (optional callable) runs between backward and the optimizer step --
    ``DataParallelTrainer`` passes its flat-bucket RCCL all-reduce, which is captured with the rest.  ``zero_grad``
    (optional callable) replaces ``optimizer.zero_grad(set_to_none=True)`` -- the data-parallel trainer's gradients are
    views of its flat bucket and must stay those tensors."""

    def __init__(self, model, criterion, optimizer, example_batch, all_reduce=None, zero_grad=None, warmup=3, clip_loss=None, **kw):
        self.model, self.criterion, self.optimizer, self.kw = model, criterion, optimizer, kw
        self.clip_loss = clip_loss or globals()['clip_loss']       # (``colour_clip_loss`` for a colour network; ``kw`` goes to it)
        self.all_reduce = all_reduce
        if zero_grad is None:
            zero_grad = self.optimizer.zero_grad if isinstance(self.optimizer, FlatAdam) else (lambda: self.optimizer.zero_grad(set_to_none=True))
        self.zero_grad = zero_grad
        self.loss = self._capture(example_batch, [(model, optimizer)], warmup)

    def _eager(self):
        input, flow, target = self.static
        self.zero_grad()
        loss, loss_sum = self.clip_loss(self.model, self.criterion, input, flow, target, **self.kw)
        backward(loss)
        if self.all_reduce is not None:
            self.all_reduce()
        self.optimizer.step()
        return loss_sum / target.shape[1]

    def __call__(self, batch):
        self._replay(batch)
        return self.loss


class GraphedAdversarialStep(_CapturedStep):
    """``adversarial_step`` (``disc_steps`` discriminator steps, then ``disc_steps`` generator steps with the discriminators switched to
    ``requires_grad_(False)``) captured ONCE in one HIP graph on one stream and replayed, as ``GraphedTrainStep``: the warm-up steps are
    undone in place -- the model, every discriminator and both optimizers are back where they were before the first replay.

    ``__call__(batch)`` -> (discr_loss, gen_loss, gt_score, pred_score) as device tensors that the next replay overwrites; nothing is
    read back.  The optimizers must be ones a capture can record: Adam built with ``capturable=True``
    (``make_adversarial_optimizers(..., capturable=True)``), or an optimizer without a host-side step count such as ``torch.optim.SGD``.
    A learning rate held as a Python float is part of the captured graph: a scheduler needs ``lr`` as a tensor.  ``kw`` goes to the two
    clip loops as in ``adversarial_step``."""

    def __init__(self, model, criterion, gen_optimizer, discr_optimizer, example_batch, disc_steps=2, warmup=2, **kw):
        if disc_steps < 1:
            raise ValueError("GraphedAdversarialStep: disc_steps must be at least 1")
        for name, opt in (("gen_optimizer", gen_optimizer), ("discr_optimizer", discr_optimizer)):
            if not all(g.get("capturable", True) for g in opt.param_groups):
                raise ValueError("GraphedAdversarialStep: %s was built with capturable=False "
                                 "(make_adversarial_optimizers(..., capturable=True))" % name)
        self.model, self.criterion, self.gen_optimizer, self.discr_optimizer = model, criterion, gen_optimizer, discr_optimizer
        self.disc_steps, self.kw = disc_steps, kw
        # (the criterion's state_dict is its discriminators': the loss modules and the shader hold no parameters or buffers)
        self.results = self._capture(example_batch, [(model, gen_optimizer), (criterion, discr_optimizer)], warmup)

    def zero_grad(self):
        self.gen_optimizer.zero_grad(set_to_none=True)
        self.discr_optimizer.zero_grad(set_to_none=True)

    def _eager(self):
        return _adversarial_step_tensors(self.model, self.criterion, self.gen_optimizer, self.discr_optimizer, self.static, self.disc_steps,
                                         **self.kw)

    def __call__(self, batch):
        self._replay(batch)
        return self.results


class DataParallelTrainer:
    """Data-parallel ``train_step``: one process per GPU, one flat gradient all-reduce per step.

    Every parameter's ``.grad`` IS a view of the flat bucket (set once here): backward accumulates straight into it
    (autograd adds in place into an existing ``.grad``; the deferred weight-gradient pass does ``grad.add_``), so the
    exchange is ONE ``all_reduce`` + ONE ``div_`` and zeroing the gradients ONE ``zero_`` -- no per-parameter copies
    around a 42 us collective.  Nothing may replace ``param.grad`` afterwards: use ``trainer.zero_grad()``, never
    ``optimizer.zero_grad()`` (whose default sets the gradients to None).

    A batch-norm generator (``useBN``): batch statistics and running statistics are PER RANK and not synchronised -- every rank
    normalises with its own shard's statistics and keeps its own running mean and variance; only the gradients are exchanged."""

    def __init__(self, model, criterion, optimizer, process_group=None):
        self.model, self.criterion, self.optimizer = model, criterion, optimizer
        self.group = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        self.params = [p for p in model.parameters() if p.requires_grad]
        self.numel = sum(p.numel() for p in self.params)
        first = self.params[0]
        if isinstance(optimizer, FlatAdam) and optimizer.bucket.numel() == self.numel:
            optimizer.check_views()
            self.bucket = optimizer.bucket         # the optimizer's flat gradient buffer IS the all-reduce bucket
        else:
            self.bucket = torch.zeros(self.numel, dtype=first.dtype, device=first.device)
            off = 0
            for p in self.params:
                n = p.numel()
                p.grad = self.bucket[off:off + n].view_as(p)
                off += n
        if self.world > 1:
            for p in self.params:          # identical start on every rank
                dist.broadcast(p.data, src=0, group=process_group)

    def zero_grad(self):
        self.bucket.zero_()

    def _check_views(self):
        """The gradients must still be the bucket's views (an ``optimizer.zero_grad()`` by the caller would have replaced them)."""
        base = self.bucket.data_ptr()
        off = 0
        for p in self.params:
            if p.grad is None or p.grad.data_ptr() != base + off * self.bucket.element_size():
                raise RuntimeError("DataParallelTrainer: a parameter's .grad is no longer a view of the flat bucket "
                                   "(use trainer.zero_grad(), not optimizer.zero_grad())")
            off += p.numel()

    def shard(self, batch):
        """Rank's slice of a global clip batch (B must divide evenly)."""
        if self.world == 1:
            return batch
        rank = dist.get_rank(self.group)
        B = batch[0].shape[0]
        assert B % self.world == 0, "global batch must be divisible by the number of ranks"
        per = B // self.world
        return tuple(t[rank * per:(rank + 1) * per] for t in batch)

    def _allreduce_gradients(self):
        dist.all_reduce(self.bucket, op=dist.ReduceOp.SUM, group=self.group)
        self.bucket.div_(self.world)

    def graphed(self, example_local_batch, **kw):
        """The data-parallel step captured in a HIP graph (``GraphedTrainStep``) with the flat-bucket all-reduce inside;
        needs the RCCL backend (gloo collectives cannot be captured) and an optimizer created with capturable=True."""
        return GraphedTrainStep(self.model, self.criterion, self.optimizer, example_local_batch,
                                all_reduce=self._allreduce_gradients if self.world > 1 else None,
                                zero_grad=self.zero_grad, **kw)

    def step(self, local_batch, **kw):
        input, flow, target = local_batch
        self._check_views()
        self.zero_grad()
        loss, loss_sum = clip_loss(self.model, self.criterion, input, flow, target, **kw)
        backward(loss)
        if self.world > 1:
            self._allreduce_gradients()
        self.optimizer.step()
        return float(loss_sum.item()) / target.shape[1]


# ---- the driver around the step: epochs, test pass, checkpoints, restore (mainVideoUnshaded.py:344-375, 397-473, 639-726,
# 799-826) -------------------------------------------------------------------------------------------------------------
def evaluate(model, criterion, loader, device, initial_image="zero", upscale=4, upsample="bilinear", disable_temporal=False):
    """``test(epoch)`` of mainVideoUnshaded.py:639-726: the clip recurrence without gradients over the held-out
    batches; returns ``{'total_loss', 'psnr', "('l1', 'mask')", ...}`` averaged over batches x frames, with
    ``psnr = 10 log10(1 / max(1e-10, mse_color))`` per frame (``:693``).  The reference reads every term of every frame
    back with ``.item()``; here everything is accumulated on the device and read once.  ``loader``: any iterable of batches;
    ``dataset_video.DeviceBatchLoader(test=True)`` is the fast path (no host slicing, collating or copying per batch)."""
    was_training = model.training
    model.eval()
    feed_inputs = getattr(criterion, 'uses_input', True)
    sums, frames = {}, 0

    def add(key, value):
        value = value.detach().double() if torch.is_tensor(value) else torch.tensor(float(value), dtype=torch.float64, device=device)
        sums[key] = value if key not in sums else sums[key] + value
    with torch.no_grad(), lazy_values(criterion):
        for batch in loader:
            input, flow, target = (t.to(device) for t in batch)
            for f in clip_recurrence(lambda x: model(x)[0], input, flow, target.shape[2], target, initial_image, upscale, disable_temporal,
                                     feedback=clamp_prediction, upsample=upsample if feed_inputs else None,
                                     previous_input=getattr(criterion, 'uses_previous_input', True)):
                loss0, values = criterion(target[:, f.j], f.output, f.input_high, f.previous_input, f.previous_warped_loss)
                add('total_loss', loss0)
                mse = values[('mse', 'color')]
                mse = mse.detach().double() if torch.is_tensor(mse) else torch.tensor(float(mse), dtype=torch.float64, device=device)
                add('psnr', 10.0 * torch.log10(1.0 / torch.clamp(mse, min=1e-10)))
                for key, value in values.items():
                    add(str(key), value)
                frames += 1
    model.train(was_training)
    if not frames:
        return {}
    keys = list(sums)
    host = torch.stack([sums[k] for k in keys]).cpu().tolist()       # the one read-back
    return {k: v / frames for k, v in zip(keys, host)}


def checkpoint_path(modeldir, epoch):
    return os.path.join(modeldir, "model_epoch_{}.pth".format(epoch))


def _write_checkpoint(modeldir, epoch, model, parameters, **entries):
    """``model_epoch_<epoch>.pth``: 'epoch' (the next one), the WHOLE model object, the option dict and the trainer's ``entries``."""
    os.makedirs(modeldir, exist_ok=True)
    path = checkpoint_path(modeldir, epoch)
    opt_dict = dict(parameters) if isinstance(parameters, dict) else dict(vars(parameters))      # `opt_dict = vars(opt)`, :167
    torch.save({'epoch': epoch + 1, 'model': model, 'parameters': opt_dict, **entries}, path)
    return path


def save_checkpoint(modeldir, epoch, model, parameters, optimizer, scheduler):
    """``checkpoint(epoch)`` of mainVideoUnshaded.py:799-811: the WHOLE model, optimizer and scheduler objects plus the
    option dict, keyed as ``inference.LoadedModel`` (and the reference's restore) read them."""
    return _write_checkpoint(modeldir, epoch, model, parameters, optimizer=optimizer, scheduler=scheduler)


def find_restore_epoch(modeldir, restore_epoch=-1):
    """``--restoreEpoch -1``: the last consecutively numbered ``model_epoch_N.pth`` (mainVideoUnshaded.py:350-358)."""
    if restore_epoch != -1:
        return restore_epoch
    n = 0
    while os.path.exists(checkpoint_path(modeldir, n + 1)):
        n += 1
    return n


def load_checkpoint(modeldir, restore_epoch=-1, device="cpu"):
    """``--restore`` of mainVideoUnshaded.py:344-375 -> (checkpoint dict, start epoch).  The file is read through the
    restricted unpickler of ``inference.loadedmodel``.  As in the reference the loop then starts AT the restored epoch
    number (``startEpoch = restoreEpoch``), i.e. that epoch is run again on top of its own checkpoint."""
    from .inference.loadedmodel import _CheckpointPickle
    epoch = find_restore_epoch(modeldir, restore_epoch)
    path = checkpoint_path(modeldir, epoch)
    if epoch < 1 or not os.path.exists(path):
        raise FileNotFoundError("no checkpoint to restore in %s (looked for %s)" % (modeldir, path))
    return torch.load(path, map_location=device, weights_only=False, pickle_module=_CheckpointPickle), epoch


def fit(model, criterion, train_loader, test_loader, modeldir, n_epochs, parameters, device=None, lr=1e-4, lr_step=500, lr_gamma=0.5,
        restore=False, restore_epoch=-1, graphed=None, flat_adam=False, log=print, **kw):
    """The epoch loop of mainVideoUnshaded.py:819-826 for the non-adversarial recipe:

        for epoch in range(start, n_epochs + 1):  trainNormal(epoch); test(epoch); checkpoint(epoch)

    ``trainNormal`` (:397-473) = ``scheduler.step()`` at the epoch's start, then one optimisation step per batch
    (``train_step``; on the GPU the step of a full-size batch is captured once in a HIP graph, ``GraphedTrainStep``, and
    replayed; a ragged last batch runs eagerly).  ``parameters``: the option dict / Namespace written into every
    checkpoint (``initialImage``, ``upsample``, ...; ``inference.LoadedModel`` reads it).  ``restore``: continue from
    the newest (or ``restore_epoch``) checkpoint of ``modeldir``, taking model, optimizer and scheduler from it.
    Returns (model, history) -- history = one dict per epoch with the mean training loss, the learning rate, the test
    dict of ``evaluate`` and the checkpoint path.  ``kw`` goes to ``clip_loss`` (initial_image, upscale, ...).

    ``train_loader`` / ``test_loader``: any iterables of (input, flow, target) batches.  A ``DataLoader`` over
    ``dataset_video.DatasetFromSamples`` is the reference's feed and costs more host time per batch than the captured step takes on
    the GPU; ``dataset_video.DeviceBatchLoader`` is the fast path -- the clips uploaded once, a batch one gather launch, the same split,
    order and bits (``.to(device)`` below is then a no-op; profiles/device_dataset.md)."""
    if device is None:
        device = next(model.parameters()).device
    on_gpu = str(device).startswith("cuda")
    if graphed is None:
        graphed = on_gpu
    start = 1
    if restore:
        ckpt, start = load_checkpoint(modeldir, restore_epoch, device)
        model, optimizer, scheduler = ckpt['model'].to(device), ckpt['optimizer'], ckpt['scheduler']
        if isinstance(optimizer, FlatAdam):
            optimizer.rebind()                 # parameters and gradients as views of the flat buffers again (no-op if they still are)
        log("Restore training from %s and epoch %d" % (modeldir, start))
    else:
        model = model.to(device)
        optimizer, scheduler = make_optimizer(model, lr, lr_step, lr_gamma, capturable=on_gpu and graphed, tensor_lr=on_gpu and graphed,
                                              flat=flat_adam)
    eval_kw = {k: v for k, v in kw.items() if k in ("initial_image", "upscale", "upsample", "disable_temporal")}
    history = []
    step_fn, step_shape = None, None
    for epoch in range(start, n_epochs + 1):
        lr_now = step_scheduler(optimizer, scheduler)
        model.train()
        total, batches = None, 0
        for batch in train_loader:
            batch = tuple(t.to(device, non_blocking=True) for t in batch)
            shape = tuple(tuple(t.shape) for t in batch)
            if graphed and on_gpu:
                if step_fn is None:
                    step_fn, step_shape = GraphedTrainStep(model, criterion, optimizer, batch, **kw), shape
                if shape == step_shape:
                    loss = step_fn(batch).detach().clone()
                else:
                    loss = torch.tensor(train_step(model, criterion, optimizer, batch, **kw), device=device)
            else:
                loss = torch.tensor(train_step(model, criterion, optimizer, batch, **kw))
            total = loss if total is None else total + loss
            batches += 1
        train_loss = float(total.item()) / max(1, batches) if total is not None else float('nan')
        log("===> Epoch {} Complete: Avg. Loss: {:.4f}, lr {:.3g}".format(epoch, train_loss, lr_now))
        test = evaluate(model, criterion, test_loader, device, **eval_kw) if test_loader is not None else {}
        if test:
            log("===> Avg. PSNR: {:.4f} dB".format(test['psnr']))
        path = save_checkpoint(modeldir, epoch, model, parameters, optimizer, scheduler)
        log("Checkpoint saved to {}".format(path))
        history.append({'epoch': epoch, 'train_loss': train_loss, 'lr': lr_now, 'test': test, 'checkpoint': path})
    return model, history
