#!/usr/bin/env python3
"""Generate tests/golden/deform2d_dim256_ref50.npz from the REFERENCE implementation: its 2-D module at dim = 256 (position-bias MLP of
width 64), heads 8, 8 offset groups, one bag on its hard-wired 50 x 50 grid (N = 2 500), seed 42.

Reuses make_golden.py (the stubs for the reference's unused third-party imports, the synthetic weights and inputs, the fixture format).
Every tensor is stored as make_golden.py stores it: a fixed strided subset of <= 4 096 entries plus checksums of the whole tensor (and the
fp64 oracle's distance, `noise`).  Only the six rel_pos_bias gradients are stored in full as well (`full:grad:<name>`): the projection
weights are 4 x the size they have at dim = 128, and the file has to stay below the largest existing fixture.

Usage:  python tests/golden/make_golden_dim256.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg            # noqa: E402


def case_deform2d_dim256():
    from models.DeformableAttention2D import DeformCrossAttention2D
    from oracle.deform import deform_cross_attention_2d
    torch.manual_seed(0)
    B, C, N, G = 1, 256, 2500, 8
    mod = DeformCrossAttention2D(dim=C, dim_head=64, heads=8, dropout=0.1, downsample_factor=4,
                                 offset_scale=4, offset_groups=G, offset_kernel_size=6).eval()
    params = mg.load_synth(mod, 42, "deform2d_dim256")
    x1 = mg.synth.normal((B, C, N), 42, "deform2d_dim256:x1").requires_grad_()
    x2 = mg.synth.normal((B, C, N), 42, "deform2d_dim256:x2").requires_grad_()
    w_out = mg.synth.normal((B, C, N), 42, "deform2d_dim256:wout")
    w_vg = mg.synth.normal((B * G, 2, 12, 12), 42, "deform2d_dim256:wvg")
    out, vgrid = mod(x1, x2, return_vgrid=True)
    loss = (out * w_out).sum() + (vgrid * w_vg).sum()
    loss.backward()
    a64 = x1.detach().double().requires_grad_(); b64 = x2.detach().double().requires_grad_()
    p64 = {k: v.double().requires_grad_() for k, v in params.items()}
    with mg.natural_scales() as ns:
        o64, vg64 = deform_cross_attention_2d(a64, b64, p64, grid_hw=(50, 50), offset_groups=G)
        ((o64 * w_out.double()).sum() + (vg64 * w_vg.double()).sum()).backward()
    payload = {"out": mg.summarize(out, o64), "vgrid": mg.summarize(vgrid, vg64), "loss": np.float64(loss.item()),
               "dx1": mg.summarize(x1.grad, a64.grad), "dx2": mg.summarize(x2.grad, b64.grad), **ns.payload(p64)}
    for k, g in mg.grads_of(mod).items():
        payload["grad:" + k] = mg.summarize(g, p64[k].grad)
        if "rel_pos_bias" in k:
            payload["full:grad:" + k] = g.detach().numpy()
        print(f"  d{k:<40s} reference vs fp64 oracle {mg.rel_err(g, p64[k].grad):.2e}")
    for name, a, b in (("out", out, o64), ("dx1", x1.grad, a64.grad), ("dx2", x2.grad, b64.grad)):
        print(f"  {name:<41s} reference vs fp64 oracle {mg.rel_err(a, b):.2e}")
    mg.save("deform2d_dim256_ref50", payload)


if __name__ == "__main__":
    mg.install_stubs()
    case_deform2d_dim256()
