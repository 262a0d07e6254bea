"""What the downsample-consistency tests and tests/golden/make_ds_fixtures.py share: the options, the loss specification and the inputs
of the recorded cases.  Nothing here is stored in the fixture: both sides draw the inputs from ``numpy.random.RandomState`` streams."""
import argparse
import os

import numpy as np
import torch

# (size, padding), B = 2: the border cuts a cell's centre 2 x 2 (pixel 1 zeroed, pixel 2 kept); the border is a whole cell; no border
CASES = [(16, 2), (16, 4), (8, 0)]
DS_TERMS = ("l2-ds:mask:0.7,l2-ds:normal:1.3,l2-ds:depth:0.9,l2-ds:color:1.1,"
            "l1-ds:mask:0.4,l1-ds:normal:0.6,l1-ds:depth:1.7,l1-ds:color:0.8")
LOSSES = "l1:mask:1,temp-l2:color:0.1," + DS_TERMS
RECIPE = "l1:mask:1,l1:ao:1,l1:normal:10,l1:depth:10,temp-l2:color:0.1"


def options(losses, ao=0.5, **kw):
    return argparse.Namespace(upsample='bilinear', losses=losses, lossAO=ao, lossAmbient=0.1, lossDiffuse=0.9, lossSpecular=0.0,
                              upscale_factor=4, **kw)


def uniform(seed, *shape):
    """fp32 values uniform in [-1, 1)."""
    return torch.from_numpy(np.random.RandomState(seed).uniform(-1.0, 1.0, shape).astype(np.float32))


def case_inputs(index):
    """gt, pred, input, prev_input_warped (None), prev_pred_warped of ``forward`` for case ``index``."""
    size, _ = CASES[index]
    # (the 8 x 8 case has eight cells: with the stream 420 its l2-ds:color is 0.004, below the generator's floor of 0.01 for a recorded term)
    gt, pred, inp, prev = (uniform((400, 410, 430)[index] + k, 2, c, size, size) for k, c in enumerate((6, 6, 5, 6)))
    return [gt, pred, inp, None, prev]


def reference():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ds_reference.npz"))


def check_case(index, device, fused=True):
    """Case ``index`` against the fixture: total, values, gradients of pred and prev_pred_warped, all within 1e-4."""
    from isosurfacesuperresolution_amd import losses
    ref = reference()
    size, padding = CASES[index]
    crit = losses.LossNetUnshaded(device, 5, 6, size, padding, options(LOSSES)).to(device)
    crit.fused = fused
    args = [t.to(device) if t is not None else None for t in case_inputs(index)]
    args[1].requires_grad_(True)
    args[4].requires_grad_(True)
    total, values = crit(*args)
    total.backward()
    tag = "case%d_" % index
    assert abs(total.item() - float(ref[tag + "total"])) <= 1e-4, (total.item(), float(ref[tag + "total"]))
    assert sorted(str(k) for k in values) == ref[tag + "value_keys"].tolist()
    got = np.array([float(values[k]) for k in sorted(values, key=str)])
    print("case %d: values within %.2e, total within %.2e" % (index, np.abs(got - ref[tag + "values"]).max(),
                                                             abs(total.item() - float(ref[tag + "total"]))))
    assert np.abs(got - ref[tag + "values"]).max() <= 1e-4, (got, ref[tag + "values"])
    for name, t in (("grad_pred", args[1]), ("grad_prev", args[4])):
        err = np.abs(t.grad.cpu().numpy() - ref[tag + name]).max()
        print("case %d: %s within %.2e" % (index, name, err))
        assert err <= 1e-4, (name, err)
    return crit
