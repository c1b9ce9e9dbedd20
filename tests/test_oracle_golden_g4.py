"""CPU: pins the fp64-capable oracle (oracle/deform.py) against the reference's 2-D module with TWO heads per offset group (heads 8,
offset_groups 4; tests/golden/deform2d_g4_ref50.npz from tests/golden/make_golden_g4.py).  The other 2-D fixture has one head per group;
this one pins the oracle where the position-bias MLP has two outputs.  Bounds: those of tests/test_oracle_golden.py."""
import numpy as np
import torch

from helpers import Golden, assert_zero_grad, bound_for, params_for, smml, synth
from oracle.deform import deform_cross_attention_2d

ZERO_GRADS = ("rel_pos_bias.mlp.2.bias",)   # softmax is shift invariant: this gradient is exactly 0 (noise only)


def g4_problem(device="cpu", **module_kw):
    """The fixture's module (HIP mirror, with module_kw), parameters, inputs and loss weights (tests/golden/make_golden_g4.py)."""
    B, C, N, G = 1, 128, 2500, 4
    mod = smml.DeformCrossAttention2D(dim=C, dim_head=64, heads=8, dropout=0.1, downsample_factor=4, offset_scale=4, offset_groups=G,
                                      offset_kernel_size=6, **module_kw)
    params = params_for(mod, 42, "deform2d_g4")
    x1 = synth.normal((B, C, N), 42, "deform2d_g4:x1").to(device).requires_grad_()
    x2 = synth.normal((B, C, N), 42, "deform2d_g4:x2").to(device).requires_grad_()
    w_out = synth.normal((B, C, N), 42, "deform2d_g4:wout").to(device)
    w_vg = synth.normal((B * G, 2, 12, 12), 42, "deform2d_g4:wvg").to(device)
    return mod, params, x1, x2, w_out, w_vg


def check_g4(g, out, vgrid, loss, dx1, dx2, grads, mlp_vs_fp64=False, pair_grads=None):
    """mlp_vs_fp64: the position-bias MLP's gradients that the reference's own fp32 arithmetic does not determine (the fixture carries
    their fp64 values, `sub64`: cancelling ReLU-gated sums over 1.4e6 pairs) are held to fp64 at the parity policy's max-norm bound
    (2 x the reference's own distance, tests/helpers.py) instead of to the reference's fp32 values - or, failing that, to the per-pair
    MLP kernels' gradients (pair_grads) at the bound of tests/test_gpu_regions.py (5e-4 of the scale): on this fixture the per-pair
    kernels themselves sit 1.0e-3 from fp64 on d b1 (the reference's fp32 2.6e-4)."""
    g.check("out", out); g.check("vgrid", vgrid); g.check("dx1", dx1); g.check("dx2", dx2)
    assert abs(loss - g.scalar("loss")) <= 1e-4 * abs(g.scalar("loss"))
    for k, gr in grads.items():
        if k.endswith(ZERO_GRADS):
            assert_zero_grad(f"{g.name}:d{k}", gr, g.scalar("natural:" + k))
            continue
        key = "grad:" + k
        if mlp_vs_fp64 and "rel_pos_bias" in k and g.has(key + "/sub64"):
            mine = gr.detach().double().cpu().flatten()[::int(g.array(key + "/step"))]
            s64 = torch.from_numpy(g.array(key + "/sub64")).double()
            noise = float(g.array(key + "/noise"))
            err = float((mine - s64).abs().max()) / max(float(s64.abs().max()), 1e-30)
            print(f"{g.name}:d{k}: {err:.2e} of its scale from fp64 (reference's fp32 {noise:.2e})")
            if err > bound_for(noise) and pair_grads is not None:
                ref = pair_grads[k].detach().double().cpu()
                e2 = float((gr.detach().double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)
                print(f"{g.name}:d{k}: {e2:.2e} of its scale from the per-pair kernels")
                assert e2 <= 5e-4, f"{g.name}:d{k} differs from fp64 by {err:.2e} and from the per-pair kernels by {e2:.2e}"
                continue
            assert err <= bound_for(noise), f"{g.name}:d{k} differs from fp64 by {err:.2e} > {bound_for(noise):.2e}"
            continue
        g.check(key, gr, what="d" + k)
        full = torch.from_numpy(g.array("full:grad:" + k)).double()
        noise = float(g.array("grad:" + k + "/noise")) if g.has("grad:" + k + "/noise") else None
        err = float((gr.detach().double().cpu() - full).abs().max()) / max(float(full.abs().max()), 1e-30)
        assert err <= bound_for(noise), f"{g.name}:d{k} (full tensor) differs by {err:.2e} of its scale"


def test_oracle_matches_reference_two_heads_per_group():
    g = Golden("deform2d_g4_ref50")
    _, params, x1, x2, w_out, w_vg = g4_problem()
    p = {k: v.clone().requires_grad_(v.dtype.is_floating_point) for k, v in params.items()}
    out, vgrid = deform_cross_attention_2d(x1, x2, p, grid_hw=(50, 50), offset_groups=4)
    loss = (out * w_out).sum() + (vgrid * w_vg).sum()
    loss.backward()
    check_g4(g, out, vgrid, loss.item(), x1.grad, x2.grad, {k: v.grad for k, v in p.items() if v.grad is not None})
    assert set(k for k in g.keys("full:grad:")) == {"full:grad:" + k for k in p if p[k].grad is not None}
    assert np.asarray(g.array("full:grad:rel_pos_bias.mlp.2.weight")).shape == (2, 32)
