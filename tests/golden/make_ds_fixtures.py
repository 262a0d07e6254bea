"""Generates tests/golden/ds_reference.npz: the downsample-consistency terms (`l2-ds` / `l1-ds`) of the reference's LossNetUnshaded.

The reference's Python modules (`losses`, `utils`) are IMPORTED from a checkout of the reference (its SuperresolutionNetwork directory,
given on the command line), unmodified, in the manner of make_gan_fixtures.py: torch CPU, fp32, one thread, deterministic algorithms,
an empty stand-in for `torchvision` (lossbuilder.py:6 imports it; only the VGG terms use it).  One name is bound so that the criterion
can be constructed at all: `LossBuilder.downsample_loss` names its nested class without the qualifier (lossbuilder.py:404,
`DownsampleLoss(...)` instead of `LossBuilder.DownsampleLoss(...)`) and raises NameError as shipped; here
`lossbuilder.DownsampleLoss = lossbuilder.LossBuilder.DownsampleLoss` is set as a module global first.

No inputs are stored: both sides draw them from `numpy.random.RandomState` streams (tests/ds_common.py, imported here).

Cases (ds_common.CASES), B = 2, losses ds_common.LOSSES (all eight ds terms with eight different weights, beside l1:mask and
temp-l2:color), lossAO 0.5: 16 x 16 with padding 2 (the border cuts a cell's centre 2 x 2), 16 x 16 with padding 4 (the border is a whole
cell), 8 x 8 without padding.  The reference's `pad` asserts square images when padding > 0.  Recorded per case: total, value dict, the
gradients of `pred` and of `prev_pred_warped`.

Conditions asserted on what is recorded:
  (1) every recorded number is within 4e-5 (the project's premise for its 1e-4 comparisons) of the same computation in fp64;
  (2) every ds value is at least 0.01 (a term that computes nothing cannot pass).

Run:  python tests/golden/make_ds_fixtures.py <reference checkout>/SuperresolutionNetwork
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ds_reference.npz")
PREMISE = 4e-5
sys.path.insert(0, os.path.dirname(HERE))
import ds_common as C  # noqa: E402


def main():
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "losses")):
        sys.exit("usage: make_ds_fixtures.py <reference checkout>/SuperresolutionNetwork")
    if "torchvision" not in sys.modules:
        try:
            import torchvision  # noqa: F401
        except ImportError:
            stub = types.ModuleType("torchvision")
            stub.models = types.ModuleType("torchvision.models")
            sys.modules["torchvision"], sys.modules["torchvision.models"] = stub, stub.models
    sys.path.insert(0, sys.argv[1])
    import losses
    from losses import lossbuilder
    lossbuilder.DownsampleLoss = lossbuilder.LossBuilder.DownsampleLoss

    out = {}
    worst, smallest = 0.0, np.inf

    def note(what, v32, v64):
        nonlocal worst
        d = float(np.abs(np.asarray(v32, dtype=np.float64) - np.asarray(v64, dtype=np.float64)).max())
        print("%-46s fp32 vs fp64 %.2e" % (what, d))
        worst = max(worst, d)

    for index, (size, padding) in enumerate(C.CASES):
        res = {}
        for dtype in (torch.float32, torch.float64):
            crit = losses.LossNetUnshaded(torch.device("cpu"), 5, 6, size, padding, C.options(C.LOSSES))
            if dtype == torch.float64:
                crit = crit.double()
            args = [t.to(dtype) if t is not None else None for t in C.case_inputs(index)]
            args[1].requires_grad_(True)
            args[4].requires_grad_(True)
            total, values = crit(*args)
            total.backward()
            res[dtype] = dict(total=total.item(), values=values, gpred=args[1].grad.numpy(), gprev=args[4].grad.numpy())
        r32, r64 = res[torch.float32], res[torch.float64]
        keys = sorted(r32["values"], key=str)
        tag = "case%d_" % index
        out[tag + "total"] = np.float64(r32["total"])
        out[tag + "value_keys"] = np.array([str(k) for k in keys])
        out[tag + "values"] = np.array([r32["values"][k] for k in keys], dtype=np.float64)
        out[tag + "grad_pred"], out[tag + "grad_prev"] = r32["gpred"], r32["gprev"]
        note(tag + "total", r32["total"], r64["total"])
        note(tag + "values", out[tag + "values"], [r64["values"][k] for k in keys])
        note(tag + "gradient of pred", r32["gpred"], r64["gpred"])
        note(tag + "gradient of prev_pred_warped", r32["gprev"], r64["gprev"])
        ds = [r32["values"][k] for k in keys if k[0] in ("l2-ds", "l1-ds")]
        assert len(ds) == 8, keys
        smallest = min(smallest, min(ds))
        print("    values", dict(zip(out[tag + "value_keys"].tolist(), out[tag + "values"].tolist())),
              "largest |gradient of pred| %.3g" % np.abs(r32["gpred"]).max())

    assert worst <= PREMISE, "the reference itself is %g from fp64" % worst
    assert smallest >= 0.01, "a ds value of %g" % smallest
    np.savez_compressed(OUT, **out)
    assert os.path.getsize(OUT) < 1000000, os.path.getsize(OUT)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; worst fp32-fp64 distance %.2e; smallest ds value %.3g" % (worst, smallest))


if __name__ == "__main__":
    main()
