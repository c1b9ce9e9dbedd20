"""GPU: the fused self-normalising encoder stacks of csrc/snn_stack.hip (functional.snn_stack) and the extension key `snn_fused` of MaxNet,
DeformPathomicNet, MCAT_Surv and CMTA, against plain torch in fp32 and fp64 on the CPU with the same dropout multipliers, the composed
modules, the oracles and the reference's fixtures.  Every comparison goes through helpers.assert_calibrated / assert_close / Golden.check
and lands in the parity report; the bounds are the suite's: 1e-4 of the tensor's scale, or 2 x (l2: 1.5 x) the fp32 restatement's own
distance from fp64.

Shapes: the forward runs one workgroup per (network, tile of 8 rows), a wave carries 4 output columns at a time, weight rows are read as
float4 where they are 16-byte aligned and scalar otherwise - one row (a partial tile), 3, 8 (a full tile), 9 (a tile and a row) and 20 rows
(three tiles); widths 1, 5, 7, 33, 48 (ragged column groups and lanes at every layer), 59 / 131 / 361 (unaligned weight rows), 100 / 256
(aligned); inputs that are column views of one wider tensor, the third starting at a column that is no multiple of 4; 2048 inputs with
three 256-wide layers behind them (the largest LDS footprint the kernels accept)."""
import argparse
import functools

import pytest
import torch

from helpers import Golden, assert_calibrated, assert_close, assert_zero_grad, params_for, smml, synth
from test_gpu_mcat import MODEL_KEYS, build, check_model, hip_run, oracle, with_scores
from test_mcat_host import check_against_fixture
from test_oracle_golden import ZERO_GRADS, pathomic_args

pytestmark = pytest.mark.gpu
Fh = smml.functional
P = 0.25
SIG = ((100, 256, 256), (131, 256, 256), (59, 256, 256))
# name -> (widths per network, final_relu, the inputs are column views of one tensor)
CASES = {"one": (((1, 1),), False, False), "sig": (SIG, False, True), "maxnet": (((59, 64, 48, 32, 128), (361, 64, 48, 32, 128)), True, False),
         "ragged": (((7, 33, 5, 48),), False, False), "wide": (((2048, 256, 256, 256, 256),), False, False)}
TAG = "snn"          # of the synthetic draws
SHAPES = [("one", 1), ("sig", 1), ("sig", 3), ("sig", 8), ("sig", 9), ("sig", 20), ("maxnet", 8), ("ragged", 2), ("wide", 8)]


def alpha_dropout(e, keep, p):
    """torch's AlphaDropout for the given 0 / 1 tensor: the three-term form (tests/test_snn_host.py holds it against torch's own)"""
    al = Fh.SNN_ALPHA
    A = ((al * al * p + 1) * (1 - p)) ** -0.5
    return A * keep * e + A * al * (keep - 1) + A * al * p


def make_keep(B, widths, tag):
    """0 / 1 multipliers in the flat layout of the saved activations (network-major, within a network layer by layer, dense [B, N] blocks):
    seeded draws at rate 0.25; the last row of the last block is all one, the first row of the first block all zero."""
    n = Fh.snn_keep_numel(B, widths)
    keep = (torch.rand(n, generator=torch.Generator().manual_seed(n + len(tag))) >= P).float()
    keep[n - widths[-1][-1]:] = 1.0
    keep[:widths[0][1]] = 0.0
    return keep


@functools.lru_cache(maxsize=None)
def case(name, B, with_keep, amp=0.0):
    """(xs, weights, biases, gs, keep, fp32 result, fp64 result) of plain torch on the CPU, computed once and never modified.  amp: the
    inputs are scaled so that the first layer's pre-activations reach about +-amp (0: as drawn, a few units)."""
    widths, final_relu, views = CASES[name]
    tag = f"{TAG}_{name}_{B}"
    if views:
        x_all = synth.normal((B, sum(w[0] for w in widths)), 42, tag + ":x")
        cuts = [sum(w[0] for w in widths[:g]) for g in range(len(widths) + 1)]
        xs = [x_all[:, a:b] for a, b in zip(cuts, cuts[1:])]
    else:
        x_all, xs = None, [synth.normal((B, w[0]), 42, f"{tag}:x{g}") for g, w in enumerate(widths)]
    shapes = {f"{g}.{l}.{kind}": ((n, k) if kind == "weight" else (n,)) for g, w in enumerate(widths) for l, (k, n) in enumerate(zip(w, w[1:]))
              for kind in ("weight", "bias")}
    par = synth.fill_params(shapes, 42, tag)
    ws = [[par[f"{g}.{l}.weight"] for l in range(len(w) - 1)] for g, w in enumerate(widths)]
    bs = [[par[f"{g}.{l}.bias"] for l in range(len(w) - 1)] for g, w in enumerate(widths)]
    if amp:
        with torch.no_grad():
            zmax = max(float((x.double() @ w[0].double().T).abs().max()) for x, w in zip(xs, ws))          # the biases are a few tenths
            if x_all is not None:
                x_all *= amp / zmax
            else:
                for x in xs:
                    x *= amp / zmax
    gs = [synth.normal((B, w[-1]), 42, f"{tag}:g{g}") for g, w in enumerate(widths)]
    keep = make_keep(B, widths, tag) if with_keep else None

    def run(dtype):
        res, off = {"pre_relu": [], "z0": []}, 0
        for g, (x, wl, bl) in enumerate(zip(xs, ws, bs)):
            xd = x.detach().to(dtype).clone().requires_grad_()
            wd = [t.detach().to(dtype).clone().requires_grad_() for t in wl]
            bd = [t.detach().to(dtype).clone().requires_grad_() for t in bl]
            a = xd
            for l, (W, b) in enumerate(zip(wd, bd)):
                z = a @ W.T + b
                if l == 0:
                    res["z0"].append(z.detach())
                a = torch.nn.functional.elu(z)
                if keep is not None:
                    a = alpha_dropout(a, keep[off:off + a.numel()].view(a.shape).to(dtype), P)
                off += a.numel()
            res["pre_relu"].append(a.detach())
            out = torch.relu(a) if final_relu else a
            (out * gs[g].to(dtype)).sum().backward()
            res[f"out{g}"], res[f"dx{g}"] = out.detach(), xd.grad
            for l in range(len(wd)):
                res[f"dW{g}.{l}"], res[f"db{g}.{l}"] = wd[l].grad, bd[l].grad
        return res

    return xs, ws, bs, gs, keep, run(torch.float32), run(torch.float64)


def hip(name, B, with_keep, cuda, amp=0.0, want_dx=True, det=False, stacked=False):
    widths, final_relu, views = CASES[name]
    xs, ws, bs, gs, keep, _, _ = case(name, B, with_keep, amp)
    if views:
        x_all = torch.cat(xs, dim=1).to(cuda).requires_grad_(want_dx)
        cuts = [sum(w[0] for w in widths[:g]) for g in range(len(widths) + 1)]
        xc = [x_all[:, a:b] for a, b in zip(cuts, cuts[1:])]
        assert xc[1].stride(0) == x_all.shape[1] and xc[2].storage_offset() % 4 != 0
    else:
        x_all, xc = None, [x.to(cuda).requires_grad_(want_dx) for x in xs]
    wc = [[t.to(cuda).requires_grad_() for t in wl] for wl in ws]
    bc = [[t.to(cuda).requires_grad_() for t in bl] for bl in bs]
    with smml.deterministic(det):
        outs = Fh.snn_stack(xc, wc, bc, p=P if with_keep else 0.0, keep=keep.to(cuda) if with_keep else None, final_relu=final_relu, stacked=stacked)
        sum((o * g.to(cuda)).sum() for o, g in zip(outs, gs)).backward()
    res = {}
    for g in range(len(widths)):
        res[f"out{g}"] = outs[g].detach()
        if want_dx:
            res[f"dx{g}"] = x_all.grad[:, cuts[g]:cuts[g + 1]] if views else xc[g].grad
        else:
            assert (x_all if views else xc[g]).grad is None
        for l in range(len(widths[g]) - 1):
            res[f"dW{g}.{l}"], res[f"db{g}.{l}"] = wc[g][l].grad, bc[g][l].grad
    torch.cuda.synchronize()
    return res, outs


def compare(label, res, r32, r64):
    for k, v in res.items():
        assert tuple(v.shape) == tuple(r64[k].shape), k
        assert_calibrated(f"{label} {k}", v, r32[k], r64[k])


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("with_keep", [False, True], ids=["plain", "keep"])
@pytest.mark.parametrize("name, B", SHAPES)
def test_stack_against_fp64(cuda, name, B, with_keep):
    _, _, _, _, keep, r32, r64 = case(name, B, with_keep)
    if CASES[name][1]:          # the final ReLU is a decision: no pre-ReLU value of the fp64 run within 1e-4 of the kink (change TAG, not the bound)
        assert min(float(a.abs().min()) for a in r64["pre_relu"]) > 1e-4
    res, outs = hip(name, B, with_keep, cuda)
    compare(f"snn {name} B{B}{' keep' if with_keep else ''}", res, r32, r64)
    last = {w[-1] for w in CASES[name][0]}
    if len(last) == 1:          # the outputs are the slices of one contiguous [G, B, N] tensor
        n = B * last.pop()
        assert all(o.is_contiguous() and o.data_ptr() == outs[0].data_ptr() + 4 * g * n for g, o in enumerate(outs))


@pytest.mark.parametrize("with_keep", [False, True], ids=["plain", "keep"])
def test_without_input_gradients_nothing_else_changes(cuda, with_keep):
    a, _ = hip("sig", 9, with_keep, cuda, want_dx=True)
    b, _ = hip("sig", 9, with_keep, cuda, want_dx=False)          # asserts that no input gradient exists
    assert set(a) - set(b) == {"dx0", "dx1", "dx2"}
    for k, v in b.items():
        assert torch.equal(v, a[k]), k


def test_stacked_output_is_the_same_tensor(cuda):
    a, outs = hip("sig", 9, True, cuda)
    b, st = hip("sig", 9, True, cuda, stacked=True)
    assert tuple(st.shape) == (3, 9, 256) and st.is_contiguous()
    for k, v in a.items():
        assert torch.equal(v, b[k]), k


@pytest.mark.parametrize("name, B", [("sig", 20), ("maxnet", 8)])
def test_runs_are_identical_and_deterministic_mode_changes_nothing(cuda, name, B):
    a, _ = hip(name, B, True, cuda)
    b, _ = hip(name, B, True, cuda)
    c, _ = hip(name, B, True, cuda, det=True)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k} differs between two runs"
        assert torch.equal(a[k], c[k]), f"{k} differs inside deterministic()"


@pytest.mark.parametrize("amp", [100.0, 1e4])
@pytest.mark.parametrize("with_keep", [False, True], ids=["plain", "keep"])
def test_saturated_elu(cuda, amp, with_keep):
    """First-layer pre-activations of +-100 and +-1e4: expm1 saturates at -1, nothing overflows, and the gradient through a saturated unit is
    exactly zero (elu' = e + 1)."""
    _, _, _, _, _, r32, r64 = case("sig", 1, with_keep, amp)
    assert 0.99 * amp < max(float(z.abs().max()) for z in r64["z0"]) < 1.01 * amp
    res, _ = hip("sig", 1, with_keep, cuda, amp=amp)
    assert all(bool(torch.isfinite(v).all()) for v in res.values())
    compare(f"snn saturated {amp:g}{' keep' if with_keep else ''}", res, r32, r64)
    for g, z in enumerate(r64["z0"]):
        dead = (z < -30.0).all(dim=0)          # units of layer 0 saturated in the (one) row: e = -1 exactly in fp32, so dz = 0
        assert int(dead.sum()) > 0
        assert float(res[f"dW{g}.0"][dead.to(cuda)].abs().max()) == 0.0 and float(res[f"db{g}.0"][dead.to(cuda)].abs().max()) == 0.0


def test_saturated_elu_is_minus_one(cuda):
    """One layer, no dropout: the output IS e, and it is -1 wherever the pre-activation is below -30."""
    xs, ws, bs, _, _, _, r64 = case("sig", 3, False, 1e4)
    x, w, b = xs[0].contiguous().to(cuda), ws[0][0].to(cuda), bs[0][0].to(cuda)
    (out,) = Fh.snn_stack([x], [[w]], [[b]])
    z = r64["z0"][0]
    assert bool(torch.isfinite(out).all()) and int((z < -30).sum()) > 100
    assert bool((out.cpu()[z < -30] == -1.0).all())
    assert_close("snn one layer at 1e4", out, torch.nn.functional.elu(z))


# ------------------------------------------------------------------------------------------------ MaxNet
@pytest.mark.parametrize("B", [1, 8])
def test_maxnet_fused_against_composed(cuda, B):
    net = smml.MaxNet(input_dim=59, omic_dim=32, dropout_rate=0.25, label_dim=4)
    net.load_state_dict(params_for(net, 42, "snn_maxnet"))
    net = net.to(cuda).eval()
    x = synth.normal((B, 59), 42, f"snn_maxnet:x{B}").to(cuda)
    w = synth.normal((B, 4), 42, f"snn_maxnet:w{B}").to(cuda)
    runs = {}
    for fused in (False, True):
        net.fused = fused
        net.zero_grad(set_to_none=True)
        xd = x.clone().requires_grad_()
        feats, logits, _ = net(x_omic=xd)
        ((logits * w).sum() + feats.sum()).backward()
        runs[fused] = {"features": feats.detach(), "logits": logits.detach(), "dx": xd.grad, **{"d" + k: v.grad for k, v in net.named_parameters() if v.grad is not None}}
    assert set(runs[True]) == set(runs[False]) and len(runs[True]) == 3 + 10
    for k, ref in runs[False].items():
        assert_close(f"MaxNet B{B} fused vs composed {k}", runs[True][k], ref)


def test_define_net_omic_mode_with_the_key(cuda):
    net = smml.define_net(pathomic_args(mode="omic", snn_fused=True)).to(cuda).eval()
    calls = []
    orig = Fh.snn_stack
    Fh.snn_stack = lambda *a, **k: calls.append(1) or orig(*a, **k)
    try:
        feats, logits, _ = net(x_omic=synth.normal((3, 431), 42, "snn_omic:x").to(cuda))
    finally:
        Fh.snn_stack = orig
    assert calls == [1] and tuple(feats.shape) == (3, 128) and tuple(logits.shape) == (3, 4) and float(feats.detach().min()) >= 0


# ------------------------------------------------------------------------------------------------ DeformPathomicNet
def test_pathomic_golden_with_the_key(cuda, monkeypatch):
    """DeformPathomicNet + BatchLoss + CE at N = 2500 with `snn_fused`: the reference's fixture under the checks
    test_gpu_parity.test_full_model_golden_reference_grid applies to the composed model; both MaxNets go through ONE grouped call."""
    g = Golden("pathomic_ref50")
    net = smml.DeformPathomicNet(pathomic_args(snn_fused=True))
    net.load_state_dict(params_for(net, 42, "pathomic"))
    net = net.to(cuda).eval()
    calls = []
    orig = Fh.snn_stack
    monkeypatch.setattr(Fh, "snn_stack", lambda xs, *a, **k: calls.append(len(xs)) or orig(xs, *a, **k))
    B = 2
    x_path = synth.bag(B, 2500, 1024, 42, "pathomic:bag").to(cuda)
    x_t = synth.normal((B, 59), 42, "pathomic:tumor").to(cuda)
    x_i = synth.normal((B, 361), 42, "pathomic:immune").to(cuda)
    feats, vt, vi, lg, _, _, _ = net(x_path=x_path, x_omic=None, x_omic_tumor=x_t, x_omic_immune=x_i)
    assert calls == [2], "both omic encoders in one grouped call"
    bl = smml.BatchLoss(B, 1)
    l_t, l_i = bl(lg[3], lg[4]), bl(lg[5], lg[6])
    label = torch.tensor([1, 3], device=cuda)
    loss = torch.nn.functional.cross_entropy(lg[2], label) + 0.5 * l_t.sum() + 0.5 * l_i.sum()
    loss.backward()
    g.check("features", feats); g.check("vec_t", vt); g.check("vec_i", vi); g.check("haz", lg[2])
    g.check("haz_t", lg[0]); g.check("haz_i", lg[1])
    g.check("vgrid_t", lg[4]); g.check("vgrid_i", lg[6]); g.check("batchloss_t", l_t); g.check("batchloss_i", l_i)
    g.check("omic_t_row0", lg[3][:, 0])
    assert abs(loss.item() - g.scalar("loss")) <= 1e-4 * abs(g.scalar("loss"))
    with_grad = {k for k, p in net.named_parameters() if p.grad is not None}
    assert with_grad == {k[5:] for k in g.keys("grad:")}, "set of parameters receiving a gradient differs"
    for k, p in net.named_parameters():
        if p.grad is not None and k.endswith(ZERO_GRADS):
            assert_zero_grad(f"{g.name}:d{k}", p.grad, g.scalar("natural:" + k))
        elif p.grad is not None:
            g.check("grad:" + k, p.grad, what="d" + k)


# ------------------------------------------------------------------------------------------------ MCAT_Surv
def test_mcat_golden_with_the_key(cuda):
    g = Golden("mcat_n150")
    prob, r32, r64 = oracle(2, 150)
    mod = build(cuda, prob[2], snn_fused=True).eval()
    assert mod.snn_fused and mod.mcat_fused
    res = with_scores(hip_run(mod, prob, cuda), mod, prob, cuda)
    check_against_fixture(g, res)
    check_model("snn_fused", res, r32, r64, g, MODEL_KEYS + ("A_path", "A_omic"))


def test_mcat_single_sample_with_the_key(cuda):
    prob, r32, r64 = oracle(1, 150)
    res = hip_run(build(cuda, prob[2], snn_fused=True).eval(), prob, cuda)
    assert tuple(res["logits"].shape) == (1, 4)
    for k in ("logits", "hazards", "S", "dx_omic"):
        assert_calibrated("snn_fused B = 1 " + k, res[k], r32[k], r64[k])


def test_mcat_train_mode_with_the_key(cuda):
    prob, _, _ = oracle(2, 150)
    mod = build(cuda, prob[2], snn_fused=True)
    ev = hip_run(mod.eval(), prob, cuda)
    torch.manual_seed(7)
    tr = hip_run(mod.train(), prob, cuda)
    torch.manual_seed(7)
    tr2 = hip_run(mod.train(), prob, cuda)
    assert not torch.equal(ev["logits"], tr["logits"])
    for k, v in tr.items():
        if k == "loss":
            assert v == tr2[k]
        else:
            assert bool(torch.isfinite(v).all()), k
            assert torch.equal(v, tr2[k]), f"{k} differs between two runs from the same seed"
    assert float(tr["grad:sig_networks.0.0.0.weight"].abs().max()) > 0
    opt = torch.optim.Adam(mod.parameters(), lr=1e-3)
    before = mod.sig_networks[0][0][0].weight.detach().clone()
    opt.step()
    assert not torch.equal(before, mod.sig_networks[0][0][0].weight)


def test_mcat_train_without_dropout_equals_eval_with_the_key(cuda):
    prob, _, _ = oracle(2, 150)
    mod = build(cuda, prob[2], dropout=0.0, snn_fused=True)
    for net in list(mod.sig_networks) + [mod.wsi_net]:          # the two rates the constructor does not take from `dropout`
        for m in net.modules():
            if isinstance(m, (torch.nn.Dropout, torch.nn.AlphaDropout)):
                m.p = 0.0
    ev = hip_run(mod.eval(), prob, cuda)
    tr = hip_run(mod.train(), prob, cuda)
    for k in ev:
        if k != "loss":
            assert torch.equal(ev[k], tr[k]), k
    assert ev["loss"] == tr["loss"]


# ------------------------------------------------------------------------------------------------ CMTA
@pytest.mark.parametrize("keys", [dict(snn_fused=True), dict(snn_fused=True, coattn_fused=True, coattn_fused_few_key=True)],
                         ids=["snn", "snn, few-key and few-query"])
def test_cmta_golden_with_the_key(cuda, keys):
    """CMTA at N = 150 with the sig_networks on the fused stack: the reference's fixture under the checks test_cmta_golden applies to the
    composed model."""
    from test_oracle_golden import CMTA_OUTPUTS, cmta_inputs, cmta_params
    g = Golden("cmta_n150")
    net = smml.CMTA(argparse.Namespace(label_dim=4, **keys))
    net.load_state_dict(cmta_params(net))
    net = net.to(cuda).eval()
    assert net.snn_fused is True and net.P_in_G_Att.fused_few_key is bool(keys.get("coattn_fused_few_key"))
    x_path, x_omic, w = cmta_inputs()
    xp, xo = x_path.to(cuda).requires_grad_(), x_omic.to(cuda).requires_grad_()
    out = net(x_path=xp, x_omic=xo)
    loss = (out[0] * w[0].to(cuda)).sum() + sum((out[2 + i] * w[i].to(cuda)).sum() for i in range(1, 5))
    loss.backward()
    for nm, o in zip(CMTA_OUTPUTS, out):
        g.check(nm, o)
    g.check("dx_path", xp.grad); g.check("dx_omic", xo.grad)
    assert abs(loss.item() - g.scalar("loss")) <= 1e-4 * abs(g.scalar("loss"))
    with_grad = {k for k, p in net.named_parameters() if p.grad is not None}
    assert with_grad == {k[5:] for k in g.keys("grad:")}
    for k, p in net.named_parameters():
        g.check("grad:" + k, p.grad, what="d" + k)
