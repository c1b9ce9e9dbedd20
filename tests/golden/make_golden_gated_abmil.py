#!/usr/bin/env python3
"""Generate tests/golden/gated_abmil_n300.npz from the REFERENCE implementation: its GatedABMIL (models/mil.py:102-152) on the CPU at
one bag of N = 300, label [1], seed 42, with the loss its own forward returns (CrossEntropyLoss on the sigmoid probabilities).

Reuses make_golden.py (the stubs for the reference's unused third-party imports, the synthetic weights and inputs, the fixture format).
Stored: prob, loss, the softmax over the bag, the eight parameter gradients (each with `noise`, the distance of the reference's fp32
arithmetic from the fp64 oracle tests/gated_abmil_oracle.py), the parameter names and shapes, and the natural scale sum |d s| of
d attention_weights.bias - a gradient that vanishes in exact arithmetic.  Inputs are regenerated from synth, not stored.

Usage:  python tests/golden/make_golden_gated_abmil.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg            # noqa: E402
import gated_abmil_oracle as go     # noqa: E402


def case_gated_abmil():
    from models.mil import GatedABMIL
    torch.manual_seed(0)
    mod = GatedABMIL().eval()
    x, _, labels = go.reference_problem(300)
    params = mg.load_synth(mod, 42, "gated_abmil")
    assert {k: tuple(v.shape) for k, v in params.items()} == go.PARAMS and list(params) == list(go.PARAMS)
    prob, pred, labels_out, loss = mod(x, labels, None, None)
    assert labels_out is labels and int(pred) == int(prob.argmax())
    loss.backward()
    with torch.no_grad():                # mil.py:134-138, the softmax its forward pools with
        A = F.softmax(torch.transpose(mod.attention_weights(mod.attention_V(x[0]) * mod.attention_U(x[0])), 1, 0), dim=1)[None]
    o64 = go.run_reference(x, params, labels, torch.float64)
    payload = {"prob": mg.summarize(prob, o64["prob"]), "softmax": mg.summarize(A, o64["softmax"]), "loss": np.float64(loss.item()),
               "natural:" + go.ZERO_GRAD: np.float64(o64["natural"]), "param_names": np.asarray(list(params)),
               "param_shapes": np.asarray([",".join(map(str, v.shape)) for v in params.values()])}
    for k, g in mg.grads_of(mod).items():
        payload["grad:" + k] = mg.summarize(g, None if k == go.ZERO_GRAD else o64["grad:" + k])     # no relative distance to an exact zero
        print(f"  d{k:<32s} reference vs fp64 oracle {mg.rel_err(g, o64['grad:' + k]):.2e}   (max |.| {float(g.abs().max()):.3e})")
    for name, a, b in (("prob", prob, o64["prob"]), ("softmax", A, o64["softmax"])):
        print(f"  {name:<33s} reference vs fp64 oracle {mg.rel_err(a, b):.2e}")
    print(f"  loss {loss.item():.4f}   natural scale of d{go.ZERO_GRAD}: {o64['natural']:.3e}")
    mg.save("gated_abmil_n300", payload)


if __name__ == "__main__":
    mg.install_stubs()
    case_gated_abmil()
