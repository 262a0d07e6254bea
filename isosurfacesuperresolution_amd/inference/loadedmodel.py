"""``LoadedModel``: a trained generator plus the per-frame input assembly of the viewer.

Public surface of ``SuperresolutionNetwork/inference/loadedmodel.py`` (attributes ``name, model,
unshaded, inverse_ao, initial_image_mode, input_channels`` and, for the colour networks, ``has_normal,
has_depth, input_single_channels``; ``inference(current_low, prev_high)``) for both families of generators:
the unshaded networks (mask / normal / depth in, a 6-channel G-buffer out, shaded afterwards) and the shaded
(colour) networks (RGB + mask and optionally normal and depth in, RGB out; ``loadedmodel.py:36-55,97-118``).
Differences, all additive or forced by the platform:

* flow hole filling happens on the GPU (``flowfill.fill_flow``) instead of a CPU OpenCV call
  (``loadedmodel.py:77-82``) -- no device round trip inside the frame;
* ``LoadedModel.from_model`` wraps an in-memory network (no checkpoint files ship with the
  reference, README.md:68);
* reference checkpoints pickle whole ``models.enhancenet.EnhanceNet`` objects
  (``mainVideoUnshaded.py:801``), so they cannot be read with ``weights_only=True``.  They are read through a
  RESTRICTED unpickler instead of a plain ``torch.load(weights_only=False)``: ``models.*`` / ``utils.*`` resolve to
  this package's modules (whatever top-level ``models`` the host process may have), tensors / storages / containers /
  optimizer and scheduler state resolve to torch and the standard library, and anything else is refused: names are matched as EXACT (module, name) pairs (no attribute walks), functions
  come from a fixed list, everything else must be a class defined in the module the pickle names.  A checkpoint is still code-adjacent data: load files you trust.
"""
import builtins
import importlib
import os.path
import pickle
import re

import torch


class _CheckpointPickle:
    """``pickle_module`` for ``torch.load``: ``find_class`` resolves EXACT (module, name) pairs only.

    * functions: the tensor / parameter rebuild helpers torch's own serializer emits and numpy's array reconstructors
      (``_FUNCTIONS``), nothing else -- in particular no dotted names (``torch`` + ``os.getcwd`` style attribute walks),
      and nothing that is merely *reachable* from an allowed package;
    * classes: storages / sizes / dtypes, ``collections`` containers, ``argparse.Namespace``, and CLASSES (never
      functions) defined in ``torch.nn.modules.*``, ``torch.optim.*`` and this package's ``models`` / ``utils`` /
      ``losses`` (the reference pickles whole module, optimizer and scheduler objects, ``mainVideoUnshaded.py:799-811``).
      The resolved object must be a type whose ``__module__`` is the module the pickle named, so a re-export such as
      ``torch.nn.modules.x.os`` cannot be smuggled in.
    """
    __name__ = "isosurfacesuperresolution_amd.checkpoint_pickle"
    _ALIASES = {"models": "isosurfacesuperresolution_amd.models", "utils": "isosurfacesuperresolution_amd.utils",
                "losses": "isosurfacesuperresolution_amd.losses"}
    _BUILTINS = {"set", "frozenset", "dict", "list", "tuple", "slice", "range", "complex", "int", "float", "bool",
                 "str", "bytes", "bytearray", "object"}
    _FUNCTIONS = {
        ("torch._utils", "_rebuild_tensor"), ("torch._utils", "_rebuild_tensor_v2"), ("torch._utils", "_rebuild_parameter"),
        ("torch._utils", "_rebuild_parameter_with_state"), ("torch._tensor", "_rebuild_from_type_v2"),
        ("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
        ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar"),
    }
    _CLASSES = {
        ("collections", "OrderedDict"), ("collections", "defaultdict"), ("argparse", "Namespace"),
        ("torch", "Size"), ("torch", "device"), ("torch", "Tensor"), ("torch.nn.parameter", "Parameter"),
        ("numpy", "dtype"), ("numpy", "ndarray"),
    }
    _STORAGE = re.compile(r"^(Float|Double|Half|BFloat16|Long|Int|Short|Char|Byte|Bool)Storage$")
    # packages whose CLASSES (checked below) may be named freely
    _CLASS_PACKAGES = ("torch.nn.modules.", "torch.optim.", "isosurfacesuperresolution_amd.models", "isosurfacesuperresolution_amd.utils",
                       "isosurfacesuperresolution_amd.losses", "isosurfacesuperresolution_amd.train")

    class Unpickler(pickle.Unpickler):
        def find_class(self, module, name):
            cls = _CheckpointPickle

            def refuse(why):
                raise pickle.UnpicklingError("checkpoint refers to %s.%s: %s" % (module, name, why))
            if "." in name or not name.isidentifier():
                refuse("dotted or malformed names are never resolved")
            root = module.split(".")[0]
            if root in cls._ALIASES:
                module = cls._ALIASES[root] + module[len(root):]
            if module in ("builtins", "__builtin__"):
                if name not in cls._BUILTINS:
                    refuse("refused")
                return getattr(builtins, name)
            key = (module, name)
            if key in cls._FUNCTIONS:
                return getattr(importlib.import_module(module), name)
            plain = key in cls._CLASSES or (module == "torch" and cls._STORAGE.match(name)) \
                or (module == "torch" and name in ("float32", "float64", "float16", "bfloat16", "int64", "int32", "uint8", "bool"))
            packaged = (module + ".").startswith(cls._CLASS_PACKAGES) or module in cls._CLASS_PACKAGES
            if not (plain or packaged):
                refuse("only tensors, containers, torch.nn / torch.optim classes and this package's models, utils and losses are loaded")
            obj = getattr(importlib.import_module(module), name, None)
            if obj is None:
                refuse("no such attribute")
            if isinstance(obj, torch.dtype):
                return obj
            if not isinstance(obj, type):
                refuse("not a class")
            if packaged and obj.__module__ != module:
                refuse("defined in %s, not in the module the checkpoint names" % obj.__module__)
            return obj

    load = staticmethod(pickle.load)
    dump = staticmethod(pickle.dump)
    Pickler = pickle.Pickler

from ..models import VideoTools
from ..utils import initialImage
from .flowfill import fill_flow


def guarded_forward(model, net_in):
    """``prediction, _ = model(net_in)`` with the guard contract of the HIP path around it -- what EVERY caller
    that feeds frames to a network on the device goes through (``LoadedModel.inference``, ``stats.run_clip``):

    * start of the frame: ``ops.guards_poll`` -- what the PREVIOUS frame's kernels reported (range maxima of the split-operand layers,
      the error words of the dataflow trunk and the one-launch flow fill): a plain read of pinned memory, one frame late; raises if a
      spin kernel timed out, re-routes the consumers of a layer that came close to the fp16 split's range;
    * FIRST frame of a model (``ops.range_check_due``): the synchronous check -- a layer came close to the split operands' range: exact
      routing from now on and this frame again (repeated: a fused launch only says THAT something inside it was hot, the per-layer
      pass that replaces it says where);
    * end of the frame: ``ops.guards_publish`` -- the words travel to pinned memory behind the frame's kernels.
    The caller ends a SEQUENCE with ``ops.guards_flush`` (the last frame has no successor to poll for it).  CPU tensors: the plain call."""
    if not net_in.is_cuda:
        return model(net_in)[0]
    from .. import ops
    ops.guards_poll(net_in.device)
    prediction, _ = model(net_in)
    if ops.range_check_due(net_in.device):
        for _ in range(4):
            if not ops.refresh_range_flags(net_in.device):
                break
            prediction, _ = model(net_in)
    ops.guards_publish(net_in.device)
    return prediction


class LoadedModel:
    def __init__(self, name, device, upscale_factor):
        self.name = os.path.splitext(os.path.basename(name))[0]
        self.device = device
        self.upscale_factor = upscale_factor
        checkpoint = torch.load(name, map_location=device, weights_only=False, pickle_module=_CheckpointPickle)
        parameters = checkpoint.get('parameters', dict())
        if not isinstance(parameters, dict):
            parameters = vars(parameters)
        self._setup(checkpoint['model'], parameters)

    @classmethod
    def from_model(cls, model, device, upscale_factor=4, parameters=None, name="model"):
        self = cls.__new__(cls)
        self.name = name
        self.device = device
        self.upscale_factor = upscale_factor
        self._setup(model, dict(parameters or {}))
        return self

    def _setup(self, model, parameters):
        self.parameters = parameters
        self.model = model
        self.model.to(self.device)
        self.model.train(False)
        first = self.model
        while True:   # first leaf module = first convolution (loadedmodel.py:26-34)
            children = list(first.children())
            if not children:
                break
            first = children[0]
        self.input_channels = first.in_channels
        r2 = self.upscale_factor ** 2
        self.unshaded = self.input_channels == 5 + 6 * r2 or bool(self.parameters.get('unshaded', False))
        if not self.unshaded:
            # a colour network: RGB + mask, optionally normal and depth, + the flattened previous RGB frame (loadedmodel.py:41-55)
            self.input_single_channels = self.input_channels - 3 * r2
            self.has_normal = self.input_single_channels >= 7
            if self.has_normal:
                self.input_single_channels -= 3
            self.has_depth = self.input_single_channels >= 5
            if self.has_depth:
                self.input_single_channels -= 1
        # first frame of a sequence (loadedmodel.py:58-64): colour networks start from zeros, unshaded ones from the upsampled input
        self.initial_image_mode = self.parameters.get('initialImage', 'input' if self.unshaded else 'zero')
        self.inverse_ao = self.parameters.get('aoInverted', False)
        if str(self.device).startswith("cuda"):
            from .. import ops
            ops.range_reset()             # range guard of the split-operand kernels: a new model starts unflagged

    def select_colour_input(self, current_low):
        """The colour networks' own channels of the renderer output (loadedmodel.py:98-105); the clamp exists in the first variant only."""
        if self.has_normal and self.has_depth:
            return torch.clamp(current_low[:, 0:8], 0, 1)
        if self.has_normal:
            return current_low[:, 0:7]
        if self.has_depth:
            return torch.cat((current_low[:, 0:4], current_low[:, 7:8]), dim=1)
        return current_low[:, 0:4]

    def colour_network_input(self, current_low, prev_high):
        """The colour networks' input [1, c + 48, h, w] of one frame: loadedmodel.py:97-118 up to the network call.
        ``prev_high`` [1,3,4h,4w]: the previous prediction clamped to [0, 1] (what the caller displays, mainVideo.py:416) or None; then ``initial_image_mode`` selects zeros or the x4 bilinear RGB ("unshaded" has no 3-channel form:
        ValueError, as in the reference).  The reference warps the initial image as well, so the hole-filled flow is used on the first
        frame too.  The mask channel is taken as the renderer delivers it, 0 / 1."""
        r = self.upscale_factor
        inp = self.select_colour_input(current_low)
        if prev_high is None:
            if self.initial_image_mode == "input":
                prev_high = VideoTools.upscale_bilinear(inp[:, 0:3], r)        # initialImage(.., "input") with its roundings spelled out
            else:
                prev_high = initialImage(inp, 3, self.initial_image_mode, self.inverse_ao, r)
        flow = fill_flow(current_low[:, 8:10], current_low[:, 3:4] != 0)
        previous_warped = VideoTools.warp_upscale(prev_high.to(self.device), flow, r, special_mask=False)
        return torch.cat((inp, VideoTools.flatten_high(previous_warped, r)), dim=1)

    def inference(self, current_low, prev_high):
        """current_low [1,12,h,w] renderer output (r,g,b,mask,nx,ny,nz,depth,fx,fy,ao,shadow);
        prev_high [1,6,4h,4w] previous network output or None.  Returns [1,6,4h,4w].
        Colour networks (``unshaded == False``): prev_high [1,3,4h,4w], returns the RGB prediction [1,3,4h,4w] (unclamped)."""
        with torch.no_grad():
            if not self.unshaded:
                return guarded_forward(self.model, self.colour_network_input(current_low, prev_high))
            mask = current_low[:, 3:4]
            inp = torch.cat((mask * 2 - 1, current_low[:, 4:8]), dim=1)
            if prev_high is None:
                previous_warped = initialImage(inp, 6, self.initial_image_mode, self.inverse_ao,
                                               self.upscale_factor).to(self.device)
            else:
                flow = fill_flow(current_low[:, 8:10], mask != 0)
                previous_warped = VideoTools.warp_upscale(prev_high.to(self.device), flow,
                                                          self.upscale_factor, special_mask=True)
            flat = VideoTools.flatten_high(previous_warped, self.upscale_factor)
            net_in = torch.cat((inp, flat), dim=1)
            prediction = guarded_forward(self.model, net_in)
        return prediction
