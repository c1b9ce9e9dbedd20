"""GPU tests of the attention maps of the deformable cross-attention (csrc/attn_maps.hip, smml_attn_splat_f32 of csrc/offsets.hip;
functional.deform_attention(attn_scores=...) / deform_attention_maps; return_attn_maps of the modules; attention_maps of the models).

Core level: random q, k, v, vs, gq and MLP weights; the reference is plain torch on the CPU in fp32 and fp64,
softmax(scale q k^T + cpb_mlp(signed_log(gq - vs))) (raw offsets for the raw-distance case), its column mean, and that mean splatted with
oracle.deform.sample_positions.  attn, key_mass and patch_map are compared with helpers.assert_calibrated (TOL 1e-4, 2 x the fp32 noise); no
decision is imposed: the bias is continuous across ReLU flips, the splat across cell boundaries.  Shapes: the smallest that reach each
hazard (CASES).  Further: the rows of key_mass sum to 1, nothing is negative, a patch map sums to at most 1; the splat kernel against the
same mass splatted in torch with the sampler's own corner indices and masks; run-to-run identity with and without
smml.deterministic(); the maps are those of the softmax before dropout; asking for maps changes neither `out` nor the training step.
Module level: DeformCrossAttention2D against the oracle's q, k, vs; the 1-D module; DeformCrossTransMIL / DeformPathomicNet.attention_maps."""
import argparse
import functools

import pytest
import torch

import oracle.deform as odeform
from helpers import assert_calibrated, params_for, rel_err, smml, synth

pytestmark = pytest.mark.gpu
Fh = smml.functional
NAMES = ("q", "k", "v", "vs", "gq", "w1", "b1", "w2", "b2", "w3", "b3")
SCALE = 0.125

# name -> (B, N, J, H, G, posdim, W, grid_hw of the splat, deform_attention options, expected DECISION_TAP marker)
CASES = {
    "region-one-live-row": (1, 33, 9, 8, 8, 2, 32, (5, 7), {}, "region_ids"),                  # the second 32-tile has one live row
    "region-14x14": (2, 196, 9, 8, 8, 2, 32, (14, 14), {}, "region_ids"),                    # nst = 256 > N; J no multiple of anything
    "region-700x150": (2, 700, 150, 8, 8, 2, 32, (27, 26), {}, "region_ids"),                # several tiles per workgroup, three slices
    "pair-two-heads": (2, 300, 90, 8, 4, 2, 32, (18, 17), {}, "masks2"),                     # two heads per group: group mean in the splat
    "region-two-heads": (2, 300, 90, 8, 4, 2, 32, (18, 17), {"cpb_regions_multi_head": True}, "region_ids"),
    "pair-1d": (1, 70, 40, 8, 4, 1, 32, None, {}, "masks2"),
    "region-1d": (1, 70, 40, 8, 4, 1, 32, None, {"cpb_regions": True}, "region1d_ids"),
    "pair-1d-raw": (1, 70, 40, 8, 4, 1, 32, None, {"log_distance": False}, "masks2"),
    "wide-128": (1, 70, 40, 8, 8, 2, 128, (9, 8), {}, "wide"),                                # the training form of the wide forward keeps the scores
    "one-key": (1, 40, 1, 8, 8, 2, 32, (3, 3), {}, None),                                     # key_mass = 1 up to rounding
}


def _mlp(t, dt):
    return {"rel_pos_bias.mlp.0.0.weight": t["w1"].to(dt), "rel_pos_bias.mlp.0.0.bias": t["b1"].to(dt), "rel_pos_bias.mlp.1.0.weight": t["w2"].to(dt),
            "rel_pos_bias.mlp.1.0.bias": t["b2"].to(dt), "rel_pos_bias.mlp.2.weight": t["w3"].to(dt), "rel_pos_bias.mlp.2.bias": t["b3"].to(dt)}


def probabilities(q, k, vs, gq, mlp, H, G, scale, log_distance=True, chunk=128):
    """softmax(scale q k^T + cpb_mlp(signed_log(gq - vs))) [B, H, N, J] in the dtype of its arguments (plain torch)."""
    B, N, _ = q.shape
    J, PD, o = k.shape[1], vs.shape[-1], H // G
    qh = q.view(B, N, H, -1).permute(0, 2, 1, 3) * scale
    kh = k.view(B, J, H, -1).permute(0, 2, 1, 3)
    out = []
    for i0 in range(0, N, chunk):
        i1 = min(N, i0 + chunk)
        pos = gq[None, i0:i1, None, :] - vs.view(B * G, 1, J, PD)
        bias = odeform.cpb_mlp(odeform.signed_log(pos) if log_distance else pos, mlp)                 # [(B G), i, J, o]
        bias = bias.view(B, G, i1 - i0, J, o).permute(0, 1, 4, 2, 3).reshape(B, H, i1 - i0, J)
        out.append(torch.softmax(qh[:, :, i0:i1] @ kh.transpose(-1, -2) + bias, dim=-1))
    return torch.cat(out, dim=2)


def splat(key_mass, vs, G, grid_hw, dt):
    """The group mean of key_mass [B, H, J] distributed to the grid with oracle.deform.sample_positions' corners, masks and weights, in dt.
    The integer path runs on vs as given (fp32: the sampler's own bits), the sums in dt."""
    B, H, J = key_mass.shape
    Hh, Ww = grid_hw
    m = key_mass.to(dt).view(B, G, H // G, J).mean(2).reshape(B * G, J)
    _, _, corners = odeform.sample_positions(vs[..., 0], vs[..., 1], Ww, Hh)
    out = torch.zeros(B * G, Hh * Ww, dtype=dt)
    for cx, cy, w, ok in corners:
        idx = cy.clamp(0, Hh - 1) * Ww + cx.clamp(0, Ww - 1)
        out.scatter_add_(1, idx, m * w.to(dt) * ok.to(dt))
    return out.view(B, G, Hh, Ww)


@functools.lru_cache(maxsize=None)
def problem(name):
    """Inputs and the fp32 / fp64 references of a case, computed once on the CPU and shared (read-only) by the tests."""
    B, N, J, H, G, PD, W, grid, opts, _ = CASES[name]
    gen = torch.Generator().manual_seed(7000 + N + 3 * J + W)
    rn = lambda *s: torch.randn(*s, generator=gen)
    o, sh = H // G, (32 / W) ** 0.5
    t = dict(q=rn(B, N, H * 64) * 0.4, k=rn(B, J, H * 64) * 0.4, v=rn(B, J, H * 64), vs=torch.rand(B * G, J, PD, generator=gen) * 2.4 - 1.2,
             gq=torch.rand(N, PD, generator=gen) * 2 - 1, w1=rn(W, PD) * 0.7, b1=rn(W) * 0.3, w2=rn(W, W) * 0.25 * sh, b2=rn(W) * 0.2,
             w3=rn(o, W) * 0.3 * sh, b3=rn(o) * 0.1)
    refs = {}
    for dt in (torch.float32, torch.float64):
        attn = probabilities(t["q"].to(dt), t["k"].to(dt), t["vs"].to(dt), t["gq"].to(dt), _mlp(t, dt), H, G, SCALE, opts.get("log_distance", True))
        km = attn.mean(2)
        # fp32: the sampler's coordinates are fp32 (its cells are those bits); fp64: the exact coordinates - the splat is continuous across cells
        refs[dt] = {"attn": attn, "key_mass": km, "patch_map": splat(km, t["vs"].to(dt), G, grid, dt) if grid else None}
    return t, refs


def run(name, cuda, *, maps=True, dense=True, p_drop=0.0, seed=11, grad=False, tap=None):
    """One deform_attention call of the case on the GPU -> (out, maps dict or None, q.grad or None)."""
    B, N, J, H, G, PD, W, grid, opts, _ = CASES[name]
    t, _ = problem(name)
    dev = {n: x.to(cuda).requires_grad_(grad and n != "gq") for n, x in t.items()}
    sink = Fh.AttnScores() if maps else None
    Fh.DECISION_TAP = tap
    try:
        with torch.set_grad_enabled(grad):
            out = Fh.deform_attention(*(dev[n] for n in NAMES), heads=H, groups=G, scale=SCALE, dropout_p=p_drop, dropout_seed=seed,
                                      **opts, **({"attn_scores": sink} if maps else {}))
    finally:
        Fh.DECISION_TAP = None
    res = Fh.deform_attention_maps(sink, dev["vs"], heads=H, groups=G, grid_hw=grid, dense=dense) if maps else None
    dq = None
    if grad:
        wo = torch.randn(B, N, H * 64, generator=torch.Generator().manual_seed(5)).to(cuda)
        (out * wo).sum().backward()
        dq = dev["q"].grad.detach().clone()
    torch.cuda.synchronize()
    return out.detach(), res, dq


@pytest.mark.parametrize("name", list(CASES))
def test_maps_against_plain_torch(cuda, name):
    B, N, J, H, G, PD, W, grid, opts, marker = CASES[name]
    t, refs = problem(name)
    tap = []
    out, m, _ = run(name, cuda, tap=tap)
    if marker is not None:           # the case reached the core it is about
        assert tap and tap[-1]["kind"] == "attn" and tap[-1].get(marker) is not None, f"{name}: the call did not take the expected core"
    r32, r64 = refs[torch.float32], refs[torch.float64]
    assert tuple(m["key_mass"].shape) == (B, H, J) and tuple(m["attn"].shape) == (B, H, N, J)
    assert not m["key_mass"].requires_grad and not m["attn"].requires_grad
    km = m["key_mass"].double().cpu()
    print(f"  {name}: key_mass err {rel_err(m['key_mass'], r64['key_mass']):.2e} (fp32 oracle {rel_err(r32['key_mass'], r64['key_mass']):.2e}), "
          f"attn err {rel_err(m['attn'], r64['attn']):.2e} (fp32 oracle {rel_err(r32['attn'], r64['attn']):.2e}), "
          f"max |row sum - 1| {float((km.sum(-1) - 1).abs().max()):.2e}")
    assert_calibrated(f"maps {name} attn", m["attn"], r32["attn"], r64["attn"])
    assert_calibrated(f"maps {name} key_mass", m["key_mass"], r32["key_mass"], r64["key_mass"])
    assert float((km.sum(-1) - 1).abs().max()) <= 1e-5, "a row of key_mass does not sum to 1"
    assert float(km.min()) >= 0.0 and float(m["attn"].min()) >= 0.0
    if J == 1:
        assert float((km - 1).abs().max()) <= 1e-5, "one key: key_mass must be 1 up to rounding"
    if grid is None:
        assert "patch_map" not in m, "1-D positions have no patch map"
        return
    pm = m["patch_map"]
    assert tuple(pm.shape) == (B, G, *grid) and not pm.requires_grad
    print(f"  {name}: patch_map err {rel_err(pm, r64['patch_map']):.2e} (fp32 oracle {rel_err(r32['patch_map'], r64['patch_map']):.2e}), "
          f"largest map sum {float(pm.double().sum((-1, -2)).max()):.6f}")
    assert_calibrated(f"maps {name} patch_map", pm, r32["patch_map"], r64["patch_map"])
    assert float(pm.min()) >= 0.0
    assert float(pm.double().sum((-1, -2)).max()) <= 1 + 1e-5, "a patch map sums to more than 1"
    # the splat kernel alone: the kernel's own mass, splatted in torch with the sampler's corner indices, masks and weights
    mass = m["key_mass"].cpu()
    assert_calibrated(f"maps {name} splat of the kernel's mass", pm, splat(mass, t["vs"], G, grid, torch.float32), splat(mass, t["vs"], G, grid, torch.float64))


def test_maps_without_the_dense_output(cuda):
    """dense=False (the default of the modules): the same key_mass and patch_map bit for bit, no attn."""
    _, a, _ = run("region-700x150", cuda, dense=True)
    _, b, _ = run("region-700x150", cuda, dense=False)
    assert "attn" not in b
    assert torch.equal(a["key_mass"], b["key_mass"]) and torch.equal(a["patch_map"], b["patch_map"])


@pytest.mark.parametrize("name", ["region-700x150", "pair-two-heads", "wide-128"])
def test_runs_are_bit_identical(cuda, name):
    runs = []
    for det in (False, False, True, True):
        with smml.deterministic(det):
            runs.append(run(name, cuda)[1])
    for i, r in enumerate(runs[1:], 1):
        for n in ("key_mass", "patch_map", "attn"):
            assert torch.equal(runs[0][n], r[n]), f"{n} of run {i} differs from run 0 (deterministic mode: runs 2, 3)"


@pytest.mark.parametrize("name", ["region-700x150", "pair-two-heads", "region-1d", "wide-128"])
def test_maps_are_pre_dropout_and_do_not_perturb_the_step(cuda, name):
    """Train mode with dropout 0.1: the maps are those of the softmax BEFORE dropout - the references of the p = 0 case under the same
    bound, and the p = 0 maps themselves to 1e-5 of their scale: with dropout the forward stashes each keep decision in the lowest
    mantissa bit of the score it saves (csrc/deform_common.h), which moves a score by at most one ulp, 2^-23 |score| < 4e-6 for the
    |score| < 32 of these problems; lse, formed from the moved scores, moves by no more, so a probability changes by a factor within
    exp(+-8e-6).  And the sink is passive: `out` and the gradient of q are bit-identical with and without it."""
    _, refs = problem(name)
    _, m0, _ = run(name, cuda)
    out_a, m, dq_a = run(name, cuda, p_drop=0.1, grad=True)
    out_b, _, dq_b = run(name, cuda, p_drop=0.1, grad=True, maps=False)
    assert torch.equal(out_a, out_b), "asking for maps changed the output"
    assert torch.equal(dq_a, dq_b), "asking for maps changed the gradient of q"
    r32, r64 = refs[torch.float32], refs[torch.float64]
    for n in ("attn", "key_mass") + (("patch_map",) if "patch_map" in m else ()):
        assert_calibrated(f"maps {name} p=0.1 {n}", m[n], r32[n], r64[n])
        e = rel_err(m[n], m0[n])
        print(f"  {name}: {n} with dropout vs without {e:.2e}")
        assert e <= 1e-5, f"{n} with dropout differs from the maps without by {e:.2e}"
    out_e, _, _ = run(name, cuda)
    out_f, _, _ = run(name, cuda, maps=False)
    assert torch.equal(out_e, out_f), "asking for maps changed the output of the inference call"


def test_maps_capture_in_a_graph(cuda):
    """No host synchronisation: the maps pass of a saved forward captures in a hipGraph; the replay equals the eager result."""
    name = "pair-two-heads"
    B, N, J, H, G, PD, W, grid, opts, _ = CASES[name]
    t, _ = problem(name)
    dev = {n: x.to(cuda) for n, x in t.items()}
    sink = Fh.AttnScores()
    with torch.no_grad():
        Fh.deform_attention(*(dev[n] for n in NAMES), heads=H, groups=G, scale=SCALE, attn_scores=sink, **opts)
    eager = Fh.deform_attention_maps(sink, dev["vs"], heads=H, groups=G, grid_hw=grid)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            res = Fh.deform_attention_maps(sink, dev["vs"], heads=H, groups=G, grid_hw=grid)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(res["key_mass"], eager["key_mass"]) and torch.equal(res["patch_map"], eager["patch_map"])


# ---- module level
def test_module_2d_against_the_oracle(cuda):
    """DeformCrossAttention2D(dim=128) on a 14 x 14 bag, eval: the maps against the oracle's own q, k and sample positions."""
    B, Hh, Ww, C = 2, 14, 14, 128
    N = Hh * Ww
    mod = smml.DeformCrossAttention2D(dim=C)
    params = params_for(mod, 31, "attnmaps2d")
    mod.load_state_dict(params)
    mod = mod.to(cuda).eval()
    x1, x2 = synth.normal((B, C, N), 31, "attnmaps2d:x1"), synth.normal((B, C, N), 31, "attnmaps2d:x2")
    with torch.no_grad():
        plain = mod(x1.to(cuda), x2.to(cuda))
        out, vgrid, maps = mod(x1.to(cuda), x2.to(cuda), return_vgrid=True, return_attn_maps="dense")
        out2, maps2 = mod(x1.to(cuda), x2.to(cuda), return_attn_maps=True)
    torch.cuda.synchronize()
    assert torch.equal(out, plain) and torch.equal(out2, plain), "asking for maps changed the module's output"
    assert set(maps) == {"key_mass", "patch_map", "vs", "vgrid", "attn"} and set(maps2) == {"key_mass", "patch_map", "vs", "vgrid"}
    assert torch.equal(maps["vgrid"], vgrid) and torch.equal(maps2["key_mass"], maps["key_mass"])
    H, G = mod.heads, mod.offset_groups
    refs = {}
    for dt in (torch.float32, torch.float64):
        p = {k: v.to(dt) for k, v in params.items()}
        _, _, aux = odeform.deform_cross_attention_2d(x1.to(dt), x2.to(dt), p, grid_hw=(Hh, Ww), return_aux=True)
        qx = 2.0 * torch.arange(Ww, dtype=dt) / max(Hh - 1, 1) - 1.0
        qy = 2.0 * torch.arange(Hh, dtype=dt) / max(Ww - 1, 1) - 1.0
        gq = torch.stack((qx.view(1, Ww).expand(Hh, Ww), qy.view(Hh, 1).expand(Hh, Ww)), dim=-1).reshape(N, 2)
        vs = torch.stack((aux["vsx"], aux["vsy"]), dim=-1)
        attn = probabilities(aux["q"], aux["k"], vs, gq, p, H, G, mod.scale)
        km = attn.mean(2)
        refs[dt] = {"attn": attn, "key_mass": km, "patch_map": splat(km, vs, G, (Hh, Ww), dt), "vs": vs}
    J = refs[torch.float32]["vs"].shape[1]
    assert tuple(maps["key_mass"].shape) == (B, H, J) and tuple(maps["patch_map"].shape) == (B, G, Hh, Ww) and tuple(maps["attn"].shape) == (B, H, N, J)
    for n in ("vs", "attn", "key_mass", "patch_map"):
        assert_calibrated(f"maps module 2d {n}", maps[n], refs[torch.float32][n], refs[torch.float64][n])


def _mil_args(**over):
    a = argparse.Namespace(path_dim=128, input_path_dim=64, attn_dim=2, return_vgrid=False)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_mil_attention_maps(cuda):
    torch.manual_seed(3)
    net = smml.DeformCrossTransMIL(_mil_args()).to(cuda).eval()
    B, N = 2, 144
    gen = torch.Generator().manual_seed(9)
    path, omic = torch.randn(B, N, 64, generator=gen).to(cuda), torch.randn(B, 128, generator=gen).to(cuda)
    with torch.no_grad():
        enc, logits, _ = net(path, omic)
    (enc_m, logits_m, _), maps = net.attention_maps(path, omic)
    torch.cuda.synchronize()
    assert torch.equal(enc, enc_m) and torch.equal(logits, logits_m), "attention_maps changed the forward's outputs"
    J = 3 * 3                                                   # the offset conv (kernel 6, stride 4) on a 12 x 12 grid
    assert tuple(maps["key_mass"].shape) == (B, 8, J) and tuple(maps["patch_map"].shape) == (B, 8, 12, 12)
    assert tuple(maps["vs"].shape) == (B * 8, J, 2) and tuple(maps["vgrid"].shape) == (B * 8, 2, 3, 3) and "attn" not in maps
    assert float((maps["key_mass"].double().sum(-1) - 1).abs().max()) <= 1e-5
    assert net._maps_out is None
    # with return_vgrid the forward's longer tuple comes back unchanged too
    net.args.return_vgrid = True
    with torch.no_grad():
        ref = net(path, omic)
    got, maps_v = net.attention_maps(path, omic, dense=True)
    assert len(got) == len(ref) == 5 and all(torch.equal(a, b) for a, b in zip(got, ref) if a is not None)
    assert tuple(maps_v["attn"].shape) == (B, 8, N, J) and torch.equal(maps_v["key_mass"], maps["key_mass"])
    with pytest.raises(ValueError, match="attn_dim"):
        smml.DeformCrossTransMIL(_mil_args(attn_dim=1)).to(cuda).eval().attention_maps(path, omic)


def test_pathomic_net_attention_maps(cuda):
    """The two-branch net: the forward's 7-tuple unchanged, one maps dict per branch (the branches share the bag, not the maps)."""
    from test_oracle_golden import pathomic_args
    torch.manual_seed(6)
    net = smml.DeformPathomicNet(pathomic_args(input_path_dim=64, return_vgrid=False)).to(cuda).eval()
    B, N = 2, 144
    gen = torch.Generator().manual_seed(10)
    kw = dict(x_path=torch.randn(B, N, 64, generator=gen).to(cuda), x_omic_tumor=torch.randn(B, 59, generator=gen).to(cuda),
              x_omic_immune=torch.randn(B, 361, generator=gen).to(cuda))
    with torch.no_grad():
        ref = net(**kw)
    got, maps = net.attention_maps(**kw)
    torch.cuda.synchronize()
    assert set(maps) == {"tumor", "immune"} and len(got) == len(ref) == 7
    for a, b in zip(got, ref):
        if torch.is_tensor(a):
            assert torch.equal(a, b), "attention_maps changed the forward's outputs"
    assert all(torch.equal(a, b) for a, b in zip(got[3], ref[3]))
    for m in maps.values():
        assert tuple(m["key_mass"].shape) == (B, 8, 9) and tuple(m["patch_map"].shape) == (B, 8, 12, 12)
        assert float((m["key_mass"].double().sum(-1) - 1).abs().max()) <= 1e-5 and float(m["patch_map"].min()) >= 0.0
    assert not torch.equal(maps["tumor"]["key_mass"], maps["immune"]["key_mass"])
    assert net.pathomic_net_tumor._maps_out is None and net.pathomic_net_immune._maps_out is None


def test_module_1d_has_no_patch_map(cuda):
    torch.manual_seed(5)
    mod = smml.DeformCrossAttention1D(dim=128, downsample_factor=4, offset_scale=2, offset_kernel_size=6).to(cuda).eval()
    B, n = 2, 70
    gen = torch.Generator().manual_seed(2)
    x1, x2 = torch.randn(B, n, 128, generator=gen).to(cuda), torch.randn(B, n, 128, generator=gen).to(cuda)
    with torch.no_grad():
        plain = mod.forward_tokens(x1, x2)
        out, maps = mod.forward_tokens(x1, x2, return_attn_maps="dense")
    torch.cuda.synchronize()
    J = maps["vgrid"].shape[-1]
    assert torch.equal(out, plain) and set(maps) == {"key_mass", "attn", "vs", "vgrid"}
    assert tuple(maps["key_mass"].shape) == (B, 8, J) and tuple(maps["attn"].shape) == (B, 8, n, J)
    assert rel_err(maps["attn"].mean(2), maps["key_mass"]) <= 1e-5
