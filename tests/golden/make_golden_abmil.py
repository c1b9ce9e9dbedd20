#!/usr/bin/env python3
"""Generate tests/golden/abmil_n300.npz from the REFERENCE implementation: its ABMIL (models/mil.py:34-82) on the CPU at
B = 2, N = 300, label_dim = 3, path_dim = 128, seed 42, loss = sum enc w_e + sum logits w_l with synthetic weights.

Reuses make_golden.py (the stubs for the reference's unused third-party imports, the synthetic weights and inputs, the fixture format).
Stored: the two outputs, the softmax over the bag, the eight parameter gradients (each with `noise`, the distance of the reference's fp32
arithmetic from the fp64 oracle tests/abmil_oracle.py), the parameter names and shapes, and the natural scale sum |d s| of
d attention.2.bias - a gradient that vanishes in exact arithmetic.  Inputs are regenerated from synth, not stored.

Usage:  python tests/golden/make_golden_abmil.py
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg            # noqa: E402
import abmil_oracle as ao           # noqa: E402


def case_abmil():
    from models.mil import ABMIL
    torch.manual_seed(0)
    B, N = 2, 300
    mod = ABMIL(argparse.Namespace(label_dim=3, path_dim=128)).eval()
    x, _, w_e, w_l = ao.problem(B, N)
    params = mg.load_synth(mod, 42, "abmil")
    assert {k: tuple(v.shape) for k, v in params.items()} == ao.PARAMS
    enc, logits, none = mod(x)
    assert none is None
    loss = (enc * w_e).sum() + (logits * w_l).sum()
    loss.backward()
    with torch.no_grad():
        A = F.softmax(torch.transpose(mod.attention(x), 2, 1), dim=2)       # mil.py:66-73, the softmax its forward pools with
    o64 = ao.run(x, params, w_e, w_l, torch.float64)
    payload = {"encoded": mg.summarize(enc, o64["encoded"]), "logits": mg.summarize(logits, o64["logits"]),
               "softmax": mg.summarize(A, o64["softmax"]), "loss": np.float64(loss.item()), "natural:" + ao.ZERO_GRAD: np.float64(o64["natural"]),
               "param_names": np.asarray(list(params)), "param_shapes": np.asarray([",".join(map(str, v.shape)) for v in params.values()])}
    for k, g in mg.grads_of(mod).items():
        payload["grad:" + k] = mg.summarize(g, None if k == ao.ZERO_GRAD else o64["grad:" + k])     # no relative distance to an exact zero
        print(f"  d{k:<32s} reference vs fp64 oracle {mg.rel_err(g, o64['grad:' + k]):.2e}   (max |.| {float(g.abs().max()):.3e})")
    for name, a, b in (("encoded", enc, o64["encoded"]), ("logits", logits, o64["logits"]), ("softmax", A, o64["softmax"])):
        print(f"  {name:<33s} reference vs fp64 oracle {mg.rel_err(a, b):.2e}")
    print(f"  natural scale of d{ao.ZERO_GRAD}: {o64['natural']:.3e}")
    mg.save("abmil_n300", payload)


if __name__ == "__main__":
    mg.install_stubs()
    case_abmil()
