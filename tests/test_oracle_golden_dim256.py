"""CPU: pins the fp64-capable oracle (oracle/deform.py) against the reference's 2-D module at dim = 256 - a position-bias MLP of width 64
(heads 8, 8 offset groups; tests/golden/deform2d_dim256_ref50.npz from tests/golden/make_golden_dim256.py) - and the routing of the wide
position-bias family (functional.deform_path -> 'pair_wide').  Bounds: those of tests/test_oracle_golden_g4.py.

The reference's fp32 arithmetic does not determine the MLP's gradients on this fixture (its own distance from the fp64 oracle: d W1 2.3e-4,
d b1 5.8e-4, d W2 5.5e-4, d b2 1.3e-3; everything else <= 2.7e-5): they take the `sub64` / noise rule of the parity policy."""
import numpy as np
import pytest
import torch

from helpers import Golden, assert_zero_grad, bound_for, params_for, smml, synth
from oracle.deform import deform_cross_attention_2d

Fh = smml.functional
ZERO_GRADS = ("rel_pos_bias.mlp.2.bias",)   # softmax is shift invariant: this gradient is exactly 0 (noise only)
FULL = ("rel_pos_bias.mlp.0.0.weight", "rel_pos_bias.mlp.0.0.bias", "rel_pos_bias.mlp.1.0.weight", "rel_pos_bias.mlp.1.0.bias",
        "rel_pos_bias.mlp.2.weight", "rel_pos_bias.mlp.2.bias")      # stored in full (`full:grad:`); the rest as strided summaries


def dim256_problem(device="cpu", **module_kw):
    """The fixture's module (HIP mirror, with module_kw), parameters, inputs and loss weights (tests/golden/make_golden_dim256.py)."""
    B, C, N, G = 1, 256, 2500, 8
    mod = smml.DeformCrossAttention2D(dim=C, dim_head=64, heads=8, dropout=0.1, downsample_factor=4, offset_scale=4, offset_groups=G,
                                      offset_kernel_size=6, **module_kw)
    params = params_for(mod, 42, "deform2d_dim256")
    x1 = synth.normal((B, C, N), 42, "deform2d_dim256:x1").to(device).requires_grad_()
    x2 = synth.normal((B, C, N), 42, "deform2d_dim256:x2").to(device).requires_grad_()
    w_out = synth.normal((B, C, N), 42, "deform2d_dim256:wout").to(device)
    w_vg = synth.normal((B * G, 2, 12, 12), 42, "deform2d_dim256:wvg").to(device)
    return mod, params, x1, x2, w_out, w_vg


def check_dim256(g, out, vgrid, loss, dx1, dx2, grads, mlp_vs_fp64=False):
    """The rules of test_oracle_golden_g4.check_g4 for this fixture's shapes.  mlp_vs_fp64: the position-bias MLP's gradients that the
    reference's own fp32 arithmetic does not determine (the fixture carries their fp64 values, `sub64`) are held to fp64 at the parity
    policy's max-norm bound (2 x the reference's own distance, tests/helpers.py) instead of to the reference's fp32 values."""
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
            assert err <= bound_for(noise), f"{g.name}:d{k} differs from fp64 by {err:.2e} > {bound_for(noise):.2e}"
            continue
        g.check(key, gr, what="d" + k)
        if k in FULL:
            full = torch.from_numpy(g.array("full:grad:" + k)).double()
            noise = float(g.array(key + "/noise")) if g.has(key + "/noise") else None
            err = float((gr.detach().double().cpu() - full).abs().max()) / max(float(full.abs().max()), 1e-30)
            assert err <= bound_for(noise), f"{g.name}:d{k} (full tensor) differs by {err:.2e} of its scale"


def test_oracle_matches_reference_at_dim256():
    g = Golden("deform2d_dim256_ref50")
    mod, params, x1, x2, w_out, w_vg = dim256_problem()
    assert tuple(mod.rel_pos_bias.mlp[1][0].weight.shape) == (64, 64)
    p = {k: v.clone().requires_grad_(v.dtype.is_floating_point) for k, v in params.items()}
    out, vgrid = deform_cross_attention_2d(x1, x2, p, grid_hw=(50, 50), offset_groups=8)
    loss = (out * w_out).sum() + (vgrid * w_vg).sum()
    loss.backward()
    check_dim256(g, out, vgrid, loss.item(), x1.grad, x2.grad, {k: v.grad for k, v in p.items() if v.grad is not None})
    assert set(g.keys("full:grad:")) == {"full:grad:" + k for k in FULL}
    assert np.asarray(g.array("full:grad:rel_pos_bias.mlp.1.0.weight")).shape == (64, 64)
    assert np.asarray(g.array("full:grad:rel_pos_bias.mlp.2.weight")).shape == (1, 64)


def test_modules_accept_widths_64_and_128_only():
    for dim, w in ((256, 64), (512, 128)):
        m2 = smml.DeformCrossAttention2D(dim=dim)
        m1 = smml.DeformCrossAttention1D(dim=dim)
        assert tuple(m2.rel_pos_bias.mlp[1][0].weight.shape) == tuple(m1.rel_pos_bias.mlp[1][0].weight.shape) == (w, w)
        assert tuple(m1.rel_pos_bias.mlp[2].weight.shape) == (2, w) and tuple(m1.rel_pos_bias.mlp[0][0].weight.shape) == (w, 1)
        assert m2._regions_apply(2500) is False
    for dim in (64, 192, 1024):
        with pytest.raises(NotImplementedError):
            smml.DeformCrossAttention2D(dim=dim)


@pytest.mark.parametrize("W", [64, 128])
def test_wide_widths_route_to_pair_wide(W):
    kw = dict(keys=169, w2_shape=(W, W))
    assert Fh.deform_path(posdim=2, heads=8, groups=8, w3_shape=(1, W), **kw) == "pair_wide"
    assert Fh.deform_path(posdim=2, heads=8, groups=4, w3_shape=(2, W), **kw) == "pair_wide"
    assert Fh.deform_path(posdim=1, heads=8, groups=4, w3_shape=(2, W), **kw) == "pair_wide"
    assert Fh.deform_path(posdim=1, heads=8, groups=4, w3_shape=(2, W), log_distance=False, **kw) == "pair_wide"
    # neither the region switches nor a capture change the route: no table, no pmax, no host sync is involved
    assert Fh.deform_path(posdim=2, heads=8, groups=8, w3_shape=(1, W), region_pmax_given=True, capturing=True, **kw) == "pair_wide"
    assert Fh.deform_path(posdim=2, heads=8, groups=8, w3_shape=(1, W), cpb_regions=False, **kw) == "pair_wide"
    # every mode the wide family does not have raises, naming the option: never a silent fall-back
    for opts, name in ((dict(compute_dtype="bf16"), "compute_dtype"), (dict(compute_dtype="fp16"), "compute_dtype"),
                       (dict(compute_dtype="bf16", cpb_table=True), "compute_dtype"), (dict(cpb_table=True), "cpb_table"),
                       (dict(cpb_table="forward"), "cpb_table"), (dict(cpb_regions=True), "cpb_regions"),
                       (dict(regions_multi_head=True), "cpb_regions_multi_head")):
        with pytest.raises(ValueError, match=name):
            Fh.deform_path(posdim=2, heads=8, groups=8, w3_shape=(1, W), **opts, **kw)
    with pytest.raises(ValueError, match="cpb_regions_1d"):
        Fh.deform_path(posdim=1, heads=8, groups=4, w3_shape=(2, W), cpb_regions=True, **kw)
    with pytest.raises(ValueError, match="heads // groups"):
        Fh.deform_path(posdim=2, heads=8, groups=2, w3_shape=(4, W), **kw)
    with pytest.raises(ValueError, match="w3"):
        Fh.deform_path(posdim=2, heads=8, groups=8, w3_shape=(1, 32), **kw)


def test_width_32_routing_is_unchanged():
    assert Fh.deform_path(posdim=2, heads=8, groups=8, keys=169, w2_shape=(32, 32), w3_shape=(1, 32), cpb_regions=False) == "pair"
    assert Fh.deform_path(posdim=1, heads=8, groups=4, keys=75, w2_shape=(32, 32), w3_shape=(2, 32)) == "pair"
    assert Fh.deform_path(posdim=2, heads=8, groups=8, keys=169, compute_dtype="bf16", cpb_table=True) == "table"
