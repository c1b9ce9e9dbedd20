#!/usr/bin/env python3
"""Generate tests/golden/mcat_n150.npz from the REFERENCE implementation: its MCAT_Surv (models/model.py:559-666) in eval() on the CPU at
B = 2 bags of 150 x 1024 and the 431 omic features, label_dim = 4, synthetic weights (seed 42, tag 'mcat'), loss = sum logits w.

Reuses make_golden.py (the stubs for the reference's unused third-party imports, the synthetic weights and inputs, the fixture format).
Stored, each with `noise` (the distance of the reference's fp32 arithmetic from the fp64 oracle tests/mcat_oracle.py) and at most 1024
values: logits, hazards, S; the raw scores A_coattn [2, 1, 4, 150], A_path and A_omic [2, 1, 4], captured by forward hooks; dx_omic,
dx_path and all parameter gradients; the parameter names and shapes; and the natural scale sum |d scores| of the two
attention_c.bias gradients, which vanish in exact arithmetic.  Inputs are regenerated from synth, not stored.

Usage:  python tests/golden/make_golden_mcat.py
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg            # noqa: E402
import mcat_oracle as mo            # noqa: E402


def case_mcat():
    from models.model import MCAT_Surv
    mg.MAX_KEEP = 1024
    torch.manual_seed(0)
    mod = MCAT_Surv(argparse.Namespace(label_dim=4)).eval()
    x_path, x_omic, _, w = mo.problem(2, 150)
    params = mg.load_synth(mod, 42, "mcat")
    assert {k: tuple(v.shape) for k, v in params.items()} == mo.PARAMS and list(params) == list(mo.PARAMS)
    raw = {}
    hooks = [mod.coattn.register_forward_hook(lambda m, i, o: raw.__setitem__("A_coattn", o[1])),
             mod.path_attention_head.register_forward_hook(lambda m, i, o: raw.__setitem__("A_path", o[0].permute(1, 2, 0))),
             mod.omic_attention_head.register_forward_hook(lambda m, i, o: raw.__setitem__("A_omic", o[0].permute(1, 2, 0)))]
    xp, xo = x_path.clone().requires_grad_(), x_omic.clone().requires_grad_()
    logits, hazards, S = mod(x_path=xp, x_omic=xo)
    loss = (logits * w).sum()
    loss.backward()
    for h in hooks:
        h.remove()
    o64 = mo.run(x_path, x_omic, params, w, torch.float64)
    got = {"logits": logits, "hazards": hazards, "S": S, **raw, "dx_path": xp.grad, "dx_omic": xo.grad}
    assert tuple(raw["A_coattn"].shape) == (2, 1, 4, 150) and tuple(raw["A_path"].shape) == tuple(raw["A_omic"].shape) == (2, 1, 4)
    payload = {k: mg.summarize(v, o64[k]) for k, v in got.items()}
    payload.update({"loss": np.float64(loss.item()), "param_names": np.asarray(list(params)),
                    "param_shapes": np.asarray([",".join(map(str, v.shape)) for v in params.values()])})
    for k, v in got.items():
        print(f"  {k:<60s} reference vs fp64 oracle {mg.rel_err(v, o64[k]):.2e}   (max |.| {float(v.abs().max()):.3e})")
    grads = mg.grads_of(mod)
    assert list(grads) == list(params), "every parameter receives a gradient"
    for k, g in grads.items():
        zero = k in mo.ZERO_GRADS
        payload["grad:" + k] = mg.summarize(g, None if zero else o64["grad:" + k])     # no relative distance to an exact zero
        if zero:
            payload["natural:" + k] = np.float64(o64["natural:" + k])
            print(f"  d{k:<59s} {float(g.abs().max()):.3e} against the natural scale {o64['natural:' + k]:.3e}")
        else:
            print(f"  d{k:<59s} reference vs fp64 oracle {mg.rel_err(g, o64['grad:' + k]):.2e}   (max |.| {float(g.abs().max()):.3e})")
    mg.save("mcat_n150", payload)


if __name__ == "__main__":
    mg.install_stubs()
    case_mcat()
