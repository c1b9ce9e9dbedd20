"""GPU tests of the wide position-bias family (csrc/deform_attn_wide.hip; include/smml.h smml_deform_attn_wide_*): the fp32-grade fused
core for a bias MLP of width W = 64 / 128, i.e. DeformCrossAttention2D / 1D at dim = 256 / 512.

  * the core against plain torch in fp64 with the kernels' exported ReLU decisions imposed (tests/helpers.py assert_calibrated, TOL 1e-4),
    and those decisions against the fp64 pre-activations (they may differ only where |pre-activation| < 2e-6);
  * a width-32 MLP embedded in a width-64 one against the width-32 per-pair kernels; the added channels' gradients are exactly 0;
  * run-to-run identity, with functional.deterministic() on and off;
  * the 2-D module at dim = 256 against the reference's own outputs (tests/golden/deform2d_dim256_ref50.npz), nothing imposed;
  * the 2-D module at dim = 512 and the 1-D module at dim = 256 against the oracle in fp32 / fp64 with the decisions imposed;
  * the sampler backward at 64 channels per group against torch's grid_sample in fp64;
  * a hipGraph capture of a training step at dim = 256."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import oracle.deform as odeform
from helpers import Golden, assert_calibrated, assert_zero_grad, decision_tap, params_for, smml, synth
from oracle.deform import deform_cross_attention_1d, deform_cross_attention_2d
from test_gpu_parity import _compare_param_grads, _core_reference, cpb_probe
from test_oracle_golden_dim256 import check_dim256, dim256_problem

pytestmark = pytest.mark.gpu
Fh = smml.functional
NAMES = ("q", "k", "v", "vs", "gq", "w1", "b1", "w2", "b2", "w3", "b3")


def _problem(gen, B, N, J, H, G, W, PD):
    rn = lambda *s: torch.randn(*s, generator=gen)
    o = H // G
    # weights at the scale of the width-32 tests, layer 2 shrunk by sqrt(32 / W): pre-activations of the same size at every width
    return dict(q=rn(B, N, H * 64) * 0.4, k=rn(B, J, H * 64) * 0.4, v=rn(B, J, H * 64), vs=torch.rand(B * G, J, PD, generator=gen) * 2.4 - 1.2,
                gq=torch.rand(N, PD, generator=gen) * 2 - 1, w1=rn(W, PD) * 0.7, b1=rn(W) * 0.3, w2=rn(W, W) * 0.25 * (32 / W) ** 0.5,
                b2=rn(W) * 0.2, w3=rn(o, W) * 0.3 * (32 / W) ** 0.5, b3=rn(o) * 0.1)


def _run(t, cuda, wo, H, G, p_drop=0.0, seed=3, tap=False, log_distance=True, **kw):
    dev = {n: x.to(cuda).requires_grad_(n != "gq") for n, x in t.items()}
    with (decision_tap() if tap else contextlib.nullcontext()) as tapped:
        out = Fh.deform_attention(*(dev[n] for n in NAMES), heads=H, groups=G, scale=0.125, dropout_p=p_drop, dropout_seed=seed,
                                  log_distance=log_distance, **kw)
    (out * wo).sum().backward()
    torch.cuda.synchronize()
    res = {n: dev[n].grad.detach().clone() for n in NAMES if n != "gq"} | {"out": out.detach().clone()}
    return (res, tapped.entries) if tap else res


def _reference(r, H, G, scale, keep, keep_scale, masks, raw):
    """_core_reference of tests/test_gpu_parity.py; with raw offsets (cpb_log_distance=False, 1-D) the same contract without the signed log."""
    if not raw:
        return _core_reference(*(r[n] for n in NAMES), H, G, scale, keep, keep_scale, masks=masks)
    q, k, v, vs, gq = r["q"], r["k"], r["v"], r["vs"], r["gq"]
    B, N, _ = q.shape
    J, PD, o = k.shape[1], vs.shape[-1], H // G
    p = gq[None, :, None, :] - vs.view(B * G, 1, J, PD)
    h2 = (((p @ r["w1"].T + r["b1"]) * masks[0].to(p.dtype)) @ r["w2"].T + r["b2"]) * masks[1].to(p.dtype)
    bias = (h2 @ r["w3"].T + r["b3"]).view(B, G, N, J, o).permute(0, 1, 4, 2, 3).reshape(B, H, N, J)
    d = q.shape[-1] // H
    qh = q.view(B, N, H, d).permute(0, 2, 1, 3) * scale
    kh = k.view(B, J, H, d).permute(0, 2, 1, 3)
    vh = v.view(B, J, H, d).permute(0, 2, 1, 3)
    attn = torch.softmax(qh @ kh.transpose(-1, -2) + bias, dim=-1)
    if keep is not None:
        attn = attn * (keep.to(attn.dtype) * keep_scale)
    return (attn @ vh).permute(0, 2, 1, 3).reshape(B, N, H * d)


# ---- the core against fp64 with the kernels' decisions imposed
CORE_CASES = [(2, 129, 40, 8, 8, 64, "2d", 0.0),        # ragged query and key tiles
              (1, 300, 90, 8, 4, 64, "2d", 0.25),       # two heads per group, dropout
              (1, 33, 5, 4, 2, 128, "2d", 0.0),
              (1, 1, 65, 8, 8, 128, "2d", 0.0),         # one query
              (2, 5, 1, 8, 8, 64, "2d", 0.0),           # one key
              (2, 200, 70, 8, 4, 64, "1d", 0.1),
              (1, 130, 33, 8, 4, 64, "1d-raw", 0.0)]


@pytest.mark.parametrize("B,N,J,H,G,W,pos,p_drop", CORE_CASES)
def test_core_vs_fp64_with_imposed_decisions(cuda, B, N, J, H, G, W, pos, p_drop):
    gen = torch.Generator().manual_seed(1000 + N + J)
    PD, raw = (2 if pos == "2d" else 1), pos == "1d-raw"
    t = _problem(gen, B, N, J, H, G, W, PD)
    wo = torch.randn(B, N, H * 64, generator=gen)
    seed = 17 + N
    res, tapped = _run(t, cuda, wo.to(cuda), H, G, p_drop, seed=seed, tap=True, log_distance=not raw)
    assert tapped[0]["kind"] == "attn" and tapped[0]["wide"] == W, "the call did not take the wide family"
    m1, m2 = tapped[0]["masks1"], tapped[0]["masks2"]                 # bool [(B G), N, J, W]
    assert tuple(m1.shape) == tuple(m2.shape) == (B * G, N, J, W)
    keep = Fh.deform_attention_dropout_mask(B, N, J, H, p_drop, seed, cuda) if p_drop else None
    o = H // G
    refs, nat = {}, None
    for dt in (torch.float32, torch.float64):
        r = {n: x.to(cuda, dt).requires_grad_() for n, x in t.items()}
        if dt == torch.float64:      # b3 per pair: its gradient is d bias of every pair - the natural scale of d b3 (zero in exact arithmetic)
            r["b3"] = t["b3"].to(cuda, dt).expand(B * G, N, J, o).clone().requires_grad_()
        out = _reference(r, H, G, 0.125, keep, 1.0 / (1.0 - p_drop), (m1, m2), raw)
        (out * wo.to(cuda, dt)).sum().backward()
        refs[dt] = (out, r)
    r64 = refs[torch.float64][1]
    nat = r64["b3"].grad.abs().sum((0, 1, 2))                          # [o]
    with torch.no_grad():       # the exported decisions against the exact pre-activations: they may only differ at rounding level
        p = r64["gq"][None, :, None, :] - r64["vs"].view(B * G, 1, J, PD)
        if not raw:
            p = torch.sign(p) * torch.log(p.abs() + 1)
        x1 = p @ r64["w1"].T + r64["b1"]
        x2 = torch.relu(x1) @ r64["w2"].T + r64["b2"]
        for nm, x, m in (("layer 1", x1, m1), ("layer 2", x2, m2)):
            bad = x[(x > 0) != m].abs()
            print(f"  {nm}: {bad.numel()} of {x.numel()} decisions differ from fp64" + (f", largest |pre-activation| {float(bad.max()):.2e}" if bad.numel() else ""))
            assert bad.numel() == 0 or float(bad.max()) < 2e-6, f"a {nm} decision with |pre-activation| {float(bad.max()):.2e} differs from fp64"
    tag = f"wide {B}x{N}x{J} H {H} G {G} W {W} {pos} p={p_drop}"
    assert_calibrated(tag + " out", res["out"], refs[torch.float32][0], refs[torch.float64][0])
    for n in NAMES:
        if n == "gq":
            continue
        if n == "b3":
            for oi in range(o):
                assert_zero_grad(f"{tag} db3[{oi}]", res["b3"][oi], float(nat[oi]))
            continue
        assert_calibrated(tag + " d" + n, res[n], refs[torch.float32][1][n].grad, r64[n].grad)


# ---- a width-32 MLP embedded in a width-64 one
def _without_ties(t, gen, G, cuda, margin=2e-6):
    """The problem with the sample positions of some keys redrawn until no ReLU pre-activation of the bias MLP (fp64) lies within
    `margin` of its kink.  The two kernel families evaluate the pre-activations with different arithmetic (split products on the 16-bit
    matrix pipe / exact fp32), i.e. to rounding (< 2e-6, the rule of the decision tests); a pair on the kink may then take different
    branches in the two, and ONE such pair among the 1.4e7 decisions of this shape moves d W2 by 7e-4 of its scale (measured: both
    families 2e-5 from fp64 under their own decisions).  Away from the kinks both take the fp64 branch and the comparison is about
    the arithmetic alone."""
    w1, b1, w2, b2, gq = (t[n].to(cuda, torch.float64) for n in ("w1", "b1", "w2", "b2", "gq"))
    vs = t["vs"].clone()
    for _ in range(50):
        p = gq[None, :, None, :] - vs.to(cuda, torch.float64)[:, None, :, :]
        x1 = (torch.sign(p) * torch.log(p.abs() + 1)) @ w1.T + b1
        x2 = torch.relu(x1) @ w2.T + b2
        near = (torch.minimum(x1.abs().amin(-1), x2.abs().amin(-1)) < margin).any(1).cpu()        # [(B G), J]: keys with a pair on a kink
        if not bool(near.any()):
            return dict(t, vs=vs)
        vs[near] = torch.rand(int(near.sum()), vs.shape[-1], generator=gen) * 2.4 - 1.2
    raise AssertionError("could not draw sample positions away from the ReLU kinks")


@pytest.mark.parametrize("H,G", [(8, 8), (8, 4)])
def test_embedded_narrow_mlp_matches_the_width_32_kernels(cuda, H, G):
    gen = torch.Generator().manual_seed(40 + G)
    B, N, J = 2, 300, 90
    t = _without_ties(_problem(gen, B, N, J, H, G, 32, 2), gen, G, cuda)
    wo = torch.randn(B, N, H * 64, generator=gen).to(cuda)
    o = H // G
    wide = dict(t)
    wide["w1"] = torch.cat((t["w1"], torch.zeros(32, 2)))
    wide["b1"] = torch.cat((t["b1"], -torch.ones(32)))
    wide["w2"] = torch.zeros(64, 64); wide["w2"][:32, :32] = t["w2"]
    wide["b2"] = torch.cat((t["b2"], -torch.ones(32)))
    wide["w3"] = torch.cat((t["w3"], torch.zeros(o, 32)), dim=1)
    a = _run(t, cuda, wo, H, G, 0.1, seed=5, cpb_regions=False)
    b, tapped = _run(wide, cuda, wo, H, G, 0.1, seed=5, tap=True)
    assert tapped[0].get("wide") == 64
    narrow = {"w1": b["w1"][:32], "b1": b["b1"][:32], "w2": b["w2"][:32, :32], "b2": b["b2"][:32], "w3": b["w3"][:, :32]}
    for n in a:
        if n == "b3":                                     # the sum of all d scores, zero in exact arithmetic
            continue
        got = narrow.get(n, b[n])
        scale = max(float(a[n].abs().max()), 1e-30)
        err = float((a[n] - got).abs().max()) / scale
        print(f"  H {H} G {G}: {n} {err:.2e}")
        assert err <= (2e-5 if n == "out" else 5e-4), f"{n} differs by {err:.2e} of its scale from the width-32 per-pair kernels"
    for n, extra in (("w1", b["w1"][32:]), ("b1", b["b1"][32:]), ("b2", b["b2"][32:]), ("w3", b["w3"][:, 32:]), ("w2 rows", b["w2"][32:]),
                     ("w2 columns", b["w2"][:, 32:])):
        assert float(extra.abs().max()) == 0.0, f"d{n} of the added channels is not exactly zero"


# ---- run-to-run identity
@pytest.mark.parametrize("B,N,J,H,G,W,PD", [(2, 300, 90, 8, 4, 64, 2), (1, 70, 40, 8, 8, 128, 1)])
def test_runs_are_bit_identical_with_and_without_deterministic_mode(cuda, B, N, J, H, G, W, PD):
    gen = torch.Generator().manual_seed(21)
    t = _problem(gen, B, N, J, H, G, W, PD)
    wo = torch.randn(B, N, H * 64, generator=gen).to(cuda)
    runs = []
    for det in (False, False, True, True):
        with smml.deterministic(det):
            runs.append(_run(t, cuda, wo, H, G, 0.1, seed=5))
    for i, r in enumerate(runs[1:], 1):
        for n in r:
            assert torch.equal(runs[0][n], r[n]), f"{n} of run {i} differs from run 0 (deterministic mode: runs 2, 3)"


# ---- the reference itself
def test_module_dim256_against_the_reference_golden(cuda):
    """heads 8, 8 groups, dim 256 on the reference's 50 x 50 grid: nothing imposed, the bounds of check_g4 (forward 1e-4; the MLP
    gradients that the reference's own fp32 does not determine against fp64)."""
    g = Golden("deform2d_dim256_ref50")
    mod, params, x1, x2, w_out, w_vg = dim256_problem(cuda)
    mod.load_state_dict(params)
    mod = mod.to(cuda).eval()
    with decision_tap() as tap:
        out, vgrid = mod(x1, x2, return_vgrid=True)
    tapped = tap.entries
    assert [e for e in tapped if e["kind"] == "attn"][0].get("wide") == 64, "the module took the wrong path"
    del tapped, tap
    loss = (out * w_out).sum() + (vgrid * w_vg).sum()
    loss.backward()
    torch.cuda.synchronize()
    check_dim256(g, out, vgrid, loss.item(), x1.grad, x2.grad, {k: p.grad for k, p in mod.named_parameters() if p.grad is not None},
                 mlp_vs_fp64=True)


# ---- the modules against the oracle with the kernels' decisions imposed
class WideDecisions:
    """The oracle.deform.DECISIONS interface (.cells, .relu_masks(i0, i1)) for ONE module call at width W, from its two DECISION_TAP
    entries: the sampler's cells as helpers.Decisions takes them, the ReLU decisions as the wide family exports them."""

    def __init__(self, sample_entry, attn_entry):
        vs = sample_entry["vs"]
        BG, J = vs.shape[0], vs.shape[1]
        cx, cy, _ = Fh.bilinear_corners(vs, sample_entry["Hh"], sample_entry["Ww"], sample_entry["posdim"])
        self.cells = (cx[:, 0].reshape(BG, J).long().cpu(), cy[:, 0].reshape(BG, J).long().cpu())
        assert attn_entry.get("wide") in (64, 128) and attn_entry["masks1"].shape[0] == BG
        self.m1, self.m2 = attn_entry["masks1"].cpu(), attn_entry["masks2"].cpu()         # bool [(B G), N, J, W]

    def relu_masks(self, i0, i1, device="cpu"):
        return self.m1[:, i0:i1].to(device), self.m2[:, i0:i1].to(device)


def _wide_decisions(tap):
    e = tap.entries
    assert len(e) == 2 and e[0]["kind"] == "sample" and e[1]["kind"] == "attn"
    return WideDecisions(e[0], e[1])


class _attend_with_keep:
    """The 1-D oracle has no dropout argument: inside the block its attention takes this keep mask (oracle.deform._attend's own argument)."""

    def __init__(self, keep, p):
        self.keep, self.p = keep, p

    def __enter__(self):
        self.orig = odeform._attend
        if self.keep is not None:
            odeform._attend = lambda q, k, v, bias_fn, heads, scale, q_chunk: self.orig(q, k, v, bias_fn, heads, scale, q_chunk, self.keep,
                                                                                        1.0 / (1.0 - self.p))

    def __exit__(self, *a):
        odeform._attend = self.orig


@pytest.mark.parametrize("kind,train", [("2d-512", True), ("2d-512", False), ("1d-256", True), ("1d-256", False)])
def test_modules_vs_oracle_with_imposed_decisions(cuda, kind, train):
    two_d = kind == "2d-512"
    if two_d:
        B, Hh, Ww, C = 2, 20, 20, 512
        n = Hh * Ww
        mod = smml.DeformCrossAttention2D(dim=C, dropout=0.1, grid_hw=(Hh, Ww))
    else:
        B, n, C = 2, 300, 256
        mod = smml.DeformCrossAttention1D(dim=C, dropout=0.1, downsample_factor=4, offset_scale=2, offset_kernel_size=6)
    tag = f"wide:{kind}"
    params = params_for(mod, 13, tag)
    mod.load_state_dict(params)
    mod = mod.to(cuda).train(train)
    x1, x2, wo = (synth.normal((B, C, n), 13, tag + s) for s in (":x1", ":x2", ":wo"))
    torch.manual_seed(1234)                                 # the dropout seed (drawn from torch's default generator)
    ad, bd = x1.to(cuda).requires_grad_(), x2.to(cuda).requires_grad_()
    with decision_tap() as tap:
        o, vg = mod(ad, bd, return_vgrid=True)
        dec = _wide_decisions(tap)
    assert tuple(mod.rel_pos_bias.mlp[1][0].weight.shape) == (C // 4, C // 4) and dec.m1.shape[-1] == C // 4
    w_vg = synth.normal(tuple(vg.shape), 13, tag + ":wvg")
    ((o * wo.to(cuda)).sum() + (vg * w_vg.to(cuda)).sum()).backward()
    J = vg.shape[-1] * vg.shape[-2] if two_d else vg.shape[-1]
    keep = Fh.deform_attention_dropout_mask(B, n, J, 8, 0.1, mod.last_dropout_seed, cuda).cpu() if train else None
    run = {}
    with cpb_probe() as probe:
        for dt in (torch.float32, torch.float64):
            pref = {k: v.clone().to(dt).requires_grad_() for k, v in params.items()}
            a, b = x1.clone().to(dt).requires_grad_(), x2.clone().to(dt).requires_grad_()
            odeform.DECISIONS = [dec]
            if two_d:
                o_ref, vg_ref = deform_cross_attention_2d(a, b, pref, grid_hw=(Hh, Ww), attn_keep=keep, dropout_p=0.1 if train else 0.0)
            else:
                with _attend_with_keep(keep, 0.1):
                    o_ref, vg_ref = deform_cross_attention_1d(a, b, pref, downsample_factor=4, offset_scale=2, offset_kernel_size=6)
            ((o_ref * wo.to(dt)).sum() + (vg_ref * w_vg.to(dt)).sum()).backward()
            run[dt] = (o_ref, vg_ref, a.grad, b.grad, pref)
    odeform.DECISIONS = None
    r32, r64 = run[torch.float32], run[torch.float64]
    for name, got, i in (("out", o, 0), ("vgrid", vg, 1), ("dx1", ad.grad, 2), ("dx2", bd.grad, 3)):
        assert_calibrated(f"{tag} train {train} {name}", got, r32[i], r64[i])
    _compare_param_grads(mod, r32[4], r64[4], probe=probe)


# ---- the sampler backward at 64 channels per offset group
@pytest.mark.parametrize("posdim", [1, 2])
@pytest.mark.parametrize("det", [False, True])
def test_sampler_backward_at_64_channels_per_group(cuda, posdim, det):
    gen = torch.Generator().manual_seed(60 + posdim)
    B, Hh, Ww, G, J, cg = 2, 9, 7, 2, 11, 64
    x = torch.randn(B, Hh, Ww, G * cg, generator=gen)
    vs = torch.rand(B * G, J, posdim, generator=gen) * 2.2 - 1.1
    wk = torch.randn(B, J, G * cg, generator=gen)
    xd, vd = x.to(cuda).requires_grad_(), vs.to(cuda).requires_grad_()
    with smml.deterministic(det):
        kv = Fh.bilinear_sample(xd, vd, groups=G, posdim=posdim)
        (kv * wk.to(cuda)).sum().backward()
    torch.cuda.synchronize()
    refs = {}
    for dt in (torch.float32, torch.float64):
        xr, vr = x.clone().to(dt).requires_grad_(), vs.clone().to(dt).requires_grad_()
        feats = xr.reshape(B, Hh, Ww, G, cg).permute(0, 3, 4, 1, 2).reshape(B * G, cg, Hh, Ww)
        grid = vr if posdim == 2 else torch.cat((vr, torch.zeros_like(vr)), dim=-1)           # (x = vs, y = 0)
        s = F.grid_sample(feats, grid.view(B * G, 1, J, 2), mode="bilinear", padding_mode="zeros", align_corners=False)   # [(B G), cg, 1, J]
        ref = s.reshape(B, G, cg, J).permute(0, 3, 1, 2).reshape(B, J, G * cg)
        (ref * wk.to(dt)).sum().backward()
        refs[dt] = (ref, xr.grad, vr.grad)
    tag = f"sampler cg 64 posdim {posdim} det {det}"
    for name, got, i in (("kv", kv, 0), ("dx", xd.grad, 1), ("dvs", vd.grad, 2)):
        assert_calibrated(f"{tag} {name}", got, refs[torch.float32][i], refs[torch.float64][i])


# ---- a captured training step
def test_training_step_at_dim256_captures_in_a_graph(cuda):
    """One eager step, then forward + backward of DeformCrossAttention2D(dim=256) captured in a hipGraph and replayed twice: no host
    synchronisation, no region table, no pmax enters the wide family.  The replays are equal to each other bit for bit (and to the eager
    step: every reduction of the step runs in a fixed order under functional.deterministic())."""
    torch.manual_seed(4)
    mod = smml.DeformCrossAttention2D(dim=256, heads=8, offset_groups=8).to(cuda).train()
    S = 12
    N = S * S
    gen = torch.Generator().manual_seed(8)
    x1, x2 = (torch.randn(1, N, 256, generator=gen) * 0.5).to(cuda), (torch.randn(1, N, 256, generator=gen) * 0.5).to(cuda)
    wo = torch.randn(1, N, 256, generator=gen).to(cuda)
    params = list(mod.parameters())

    def step():
        for p in params:
            p.grad = None
        with smml.deterministic():
            out = mod.forward_tokens(x1, x2)
            (out * wo).sum().backward()
        return out

    out_e = step().detach().clone()
    torch.cuda.synchronize()
    grads_e = [p.grad.detach().clone() for p in params]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                                        # warm-up on the capture stream
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out_g = step()
    torch.cuda.current_stream().wait_stream(s)
    replays = []
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        replays.append([out_g.detach().clone()] + [p.grad.detach().clone() for p in params])
    for a, b in zip(*replays):
        assert torch.equal(a, b), "two replays of the captured step differ"
    for a, b in zip(replays[0], [out_e] + grads_e):
        assert torch.equal(a, b), "the replayed step differs from the eager step"
