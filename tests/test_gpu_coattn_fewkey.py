"""GPU: the few-key co-attention (MultiheadAttention.fused_few_key, functional.few_key_attention / coattn_few_key, csrc/fewk_attn.hip)
against the reference's fixture coattn_L2500_S4 and against oracle.coattn.coattention run on the CPU in fp32 and fp64.  Every comparison goes
through helpers.assert_calibrated / assert_close / Golden.check and lands in the parity report; no tolerance of its own.

Every loss carries the raw-score term of test_coattention_golden, (raw w_r).sum() 1e-2 over the finite entries: without it the query third
of in_proj_bias has no gradient (softmax is shift invariant).

Shapes: a workgroup walks tiles of 16 rows inside its split, one row per 16-lane group, four rows per wave.  L = 11 is less than one tile,
16 exactly one, 37 two tiles and a ragged third of 5 rows in one split; 300 rows cut into 7 splits of 43 end in a split of 42 rows and every
split ends in a ragged tile; 300 splits hold one row each.  S = 1, 3, 4 take the four-key register layout, S = 8 the eight-key one, whose
backward runs as two launches (dx / du / dc, then dw)."""
import argparse
import functools

import pytest
import torch

from helpers import Golden, assert_calibrated, assert_close, params_for, smml, synth
from oracle.coattn import coattention

pytestmark = pytest.mark.gpu
Fh = smml.functional
E = 256
PARAMS = ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias")
KEYS = ("out", "raw", "dq", "dk", "dv") + tuple("grad:" + k for k in PARAMS)


def mask_for(B, S):
    """a different key in each bag: key b of bag b"""
    kpm = torch.zeros(B, S, dtype=torch.bool)
    for b in range(B):
        kpm[b, b % S] = True
    return kpm


@functools.lru_cache(maxsize=None)
def problem(B, S, L, variant=""):
    """(q [L, B, E] - the bag -, k [S, B, E], v or None (the values are the keys), params, w_o, w_r, key_padding_mask or None); never modified"""
    tag = f"fewk_{B}_{S}_{L}"
    params = params_for(smml.MultiheadAttention(E, 1), 42, tag)
    q, k = synth.normal((L, B, E), 42, tag + ":q"), synth.normal((S, B, E), 42, tag + ":kv")
    v = synth.normal((S, B, E), 42, tag + ":v") if variant == "kv" else None
    kpm = mask_for(B, S) if variant == "masked" else None
    if variant == "peaked":
        q = peaked(q, k, params)
    return q, k, v, params, synth.normal((L, B, E), 42, tag + ":wo"), synth.normal((B, 1, L, S), 42, tag + ":wr"), kpm


def scores(q, k, params):
    p = {n: t.double() for n, t in params.items()}
    w, b = p["in_proj_weight"], p["in_proj_bias"]
    return torch.einsum("lbe,sbe->bls", (q.double() @ w[:E].t() + b[:E]) * E ** -0.5, k.double() @ w[E:2 * E].t() + b[E:2 * E])


def peaked(q, k, params):
    """The queries scaled until the S scores of the median row spread over 60 units: almost every row's softmax is one-hot to fp32."""
    r = scores(q, k, params)
    return q * float(60.0 / (r.max(-1).values - r.min(-1).values).median())


def finite(raw):
    return torch.where(torch.isfinite(raw), raw, torch.zeros_like(raw))


def loss_of(out, raw, w_o, w_r):
    return (out * w_o).sum() + (finite(raw) * w_r).sum() * 1e-2


@functools.lru_cache(maxsize=None)
def oracle(B, S, L, variant=""):
    """(fp32, fp64) evaluations of oracle.coattn.coattention on the CPU, computed once per problem and shared"""
    q, k, v, params, w_o, w_r, kpm = problem(B, S, L, variant)
    res = []
    for dt in (torch.float32, torch.float64):
        leaf = lambda t: t.detach().clone().to(dt).requires_grad_()          # noqa: E731
        ql, kl = leaf(q), leaf(k)
        vl = leaf(v) if v is not None else kl
        p = {n: leaf(t) for n, t in params.items()}
        out, raw = coattention(ql, kl, vl, p, key_padding_mask=kpm)
        loss_of(out, raw, w_o.to(dt), w_r.to(dt)).backward()
        r = {"out": out.detach(), "raw": finite(raw).detach(), "masked": ~torch.isfinite(raw), "softmax": torch.softmax(raw.detach()[:, 0], -1),
             "dq": ql.grad, "dk": kl.grad, "dv": vl.grad if v is not None else None}
        r.update({"grad:" + n: t.grad for n, t in p.items()})
        res.append(r)
    return tuple(res)


def module(params, cuda, splits=None, fused=True):
    mod = smml.MultiheadAttention(E, 1)
    mod.load_state_dict(params)
    mod.fused_few_key, mod.fewk_splits = fused, splits
    return mod.to(cuda).eval()


def hip_run(prob, cuda, splits=None, det=False, q_grad=True, fused=True):
    q, k, v, params, w_o, w_r, kpm = prob
    mod = module(params, cuda, splits, fused)
    qd, kd = q.to(cuda).requires_grad_(q_grad), k.to(cuda).requires_grad_()
    vd = v.to(cuda).requires_grad_() if v is not None else kd
    with smml.deterministic(det):
        # the two transposes of CMTA's call: key and value are two views of one tensor
        out, raw = mod(qd, kd.transpose(0, 1).transpose(0, 1), vd.transpose(0, 1).transpose(0, 1), key_padding_mask=kpm.to(cuda) if kpm is not None else None)
        assert tuple(out.shape) == tuple(q.shape) and tuple(raw.shape) == (q.shape[1], 1, q.shape[0], k.shape[0])
        loss_of(out, raw, w_o.to(cuda), w_r.to(cuda)).backward()
    torch.cuda.synchronize()
    if q_grad:
        assert qd.grad.is_contiguous(), "query.grad is dense in the query's own (sequence-first) layout"
    res = {"out": out.detach(), "raw": finite(raw).detach(), "masked": ~torch.isfinite(raw.detach()), "dq": qd.grad, "dk": kd.grad,
           "dv": vd.grad if v is not None else None}
    res.update({"grad:" + n: t.grad for n, t in mod.named_parameters()})
    return res


def check(name, res, r32, r64, keys=KEYS):
    for key in keys:
        if r64[key] is None:
            continue
        assert tuple(res[key].shape) == tuple(r64[key].shape), key
        assert_calibrated(f"{name} {key}", res[key], r32[key], r64[key])


def test_golden_parity(cuda):
    """The reference's own output at the reference's shape, flag on, the library's split count - checked as test_coattention_golden checks
    the composed path."""
    tag, L, S, B = "coattn_L2500_S4", 2500, 4, 2
    g = Golden(tag)
    mod = module(params_for(smml.MultiheadAttention(E, 1), 42, tag), cuda)
    q = synth.normal((L, B, 256), 42, tag + ":q").to(cuda).requires_grad_()
    kv = synth.normal((S, B, 256), 42, tag + ":kv").to(cuda).requires_grad_()
    w_o = synth.normal((L, B, 256), 42, tag + ":wo").to(cuda); w_r = synth.normal((B, 1, L, S), 42, tag + ":wr").to(cuda)
    assert Fh.coattn_few_key_why(S=S, heads=1, Eq=E, fused=mod.fused_few_key) is None
    out, raw = mod(q, kv, kv)
    assert out.shape == (L, B, 256) and raw.shape == (B, 1, L, S)
    ((out * w_o).sum() + (raw * w_r).sum() * 1e-2).backward()
    g.check("out", out); g.check("raw", raw); g.check("dq", q.grad); g.check("dkv", kv.grad)
    for k, p in mod.named_parameters():
        g.check("grad:" + k, p.grad, what="d" + k)


@pytest.mark.parametrize("B, S, L, splits", [(3, 4, 11, None), (1, 1, 16, 1), (3, 3, 37, 1), (3, 4, 300, 7), (1, 8, 300, 7), (3, 8, 37, None),
                                             (1, 3, 300, 300), (3, 1, 300, 7)])
def test_ragged_shapes(cuda, B, S, L, splits):
    check(f"ragged {B}x{S}x{L} splits {splits}", hip_run(problem(B, S, L), cuda, splits=splits), *oracle(B, S, L))


def test_split_counts_agree(cuda):
    runs = {s: hip_run(problem(3, 4, 300), cuda, splits=s) for s in (1, 2, 7)}
    for s in (2, 7):
        for key in KEYS:
            if runs[1][key] is not None:
                assert_close(f"splits {s} vs 1 {key}", runs[s][key], runs[1][key])
        assert torch.equal(runs[s]["out"], runs[1]["out"]) and torch.equal(runs[s]["raw"], runs[1]["raw"]), "no sum crosses rows in the forward"


def test_key_padding_mask(cuda):
    B, S, L = 3, 4, 300
    prob, (r32, r64) = problem(B, S, L, "masked"), oracle(B, S, L, "masked")
    kpm = prob[6]
    res = hip_run(prob, cuda, splits=7)
    assert int(res["masked"].sum()) == int(r64["masked"].sum()) == L * B
    assert torch.equal(res["masked"].cpu(), kpm[:, None, None, :].expand(B, 1, L, S)), "raw is -inf exactly at the masked keys"
    rows = res["dk"].transpose(0, 1).cpu()[kpm]                     # [masked keys, E]: the values are the keys, the row is dk + dv
    assert rows.shape[0] == B and bool((rows == 0).all()), "gradient rows of masked keys are exactly 0"
    check("masked", res, r32, r64)
    check("masked, library splits", hip_run(prob, cuda), r32, r64)


def test_peaked_softmax(cuda):
    B, S, L = 3, 4, 300
    r32, r64 = oracle(B, S, L, "peaked")
    A, raw = r64["softmax"], r64["raw"][:, 0]
    spread = raw.max(-1).values - raw.min(-1).values
    assert 59.0 < float(spread.median()) < 61.0, "the scores of a row spread over about 60 units"
    assert float((A.max(-1).values > 1 - 1e-7).double().mean()) > 0.5, "one-hot to fp32 in more than half of the rows"
    assert float(raw.max()) > 89.0, "exp overflows in fp32 where the row maximum is not subtracted"
    check("peaked", hip_run(problem(B, S, L, "peaked"), cuda, splits=7), r32, r64)
    check("peaked, library splits", hip_run(problem(B, S, L, "peaked"), cuda), r32, r64)


def test_distinct_key_and_value(cuda):
    B, S, L = 3, 4, 300
    r32, r64 = oracle(B, S, L, "kv")
    res = hip_run(problem(B, S, L, "kv"), cuda, splits=7)
    assert res["dv"] is not None and res["dk"].data_ptr() != res["dv"].data_ptr()
    check("key != value", res, r32, r64)


def test_masked_distinct_value_rows_are_zero(cuda):
    """key != value with a mask: the masked keys' dk rows AND dv rows are exactly 0, fused against composed on everything else."""
    B, S, L = 3, 4, 37
    q, k, _, params, w_o, w_r, _ = problem(B, S, L)
    prob = (q, k, synth.normal((S, B, E), 42, "fewk_masked_v"), params, w_o, w_r, mask_for(B, S))
    res, ref = hip_run(prob, cuda), hip_run(prob, cuda, fused=False)
    for key in ("dk", "dv"):
        rows = res[key].transpose(0, 1).cpu()[prob[6]]
        assert rows.shape[0] == B and bool((rows == 0).all()), key
    for key in KEYS:
        assert_close(f"masked, key != value: fused vs composed {key}", res[key], ref[key])


@pytest.mark.parametrize("variant", ["", "kv"])
def test_query_without_gradient(cuda, variant):
    """The bag does not require a gradient: no dx buffer is formed, everything else is that of the full problem."""
    B, S, L = 3, 4, 300
    res = hip_run(problem(B, S, L, variant), cuda, splits=7, q_grad=False)
    assert res["dq"] is None
    check(f"no query gradient {variant}", res, *oracle(B, S, L, variant), keys=tuple(k for k in KEYS if k != "dq"))


def core_formula(x, u, c, w, kpm, wo, wr, dt):
    x, u, c, w = (t.detach().clone().to(dt).requires_grad_() for t in (x, u, c, w))
    raw = x @ u.transpose(1, 2) + c[:, None, :]
    if kpm is not None:
        raw = raw.masked_fill(kpm[:, None, :], float("-inf"))
    out = torch.softmax(raw, -1) @ w
    ((out * wo.to(dt)).sum() + (finite(raw) * wr.to(dt)).sum() * 1e-2).backward()
    return {"out": out.detach(), "raw": finite(raw).detach(), "dx": x.grad, "du": u.grad, "dc": c.grad, "dw": w.grad}


@pytest.mark.parametrize("Eq, Eo, S, B", [(64, 64, 3, 3), (256, 256, 4, 1), (512, 256, 8, 3), (256, 512, 3, 1), (512, 512, 4, 3)])
def test_other_widths_through_the_core(cuda, Eq, Eo, S, B):
    """few_key_attention itself, sequence-first x read in place as its transpose (strided rows), a mask, ragged splits (37 rows in 2 splits
    of 19: a full tile and 3 rows each), against the same formula on the CPU.  (512, 256, 8) is the eight-key, eight-chunk layout."""
    L = 37
    t = f"fewk_core_{Eq}_{Eo}_{S}:"
    x_sf = synth.normal((L, B, Eq), 42, t + "x")
    u, c, w = synth.normal((B, S, Eq), 42, t + "u") * 0.3, synth.normal((B, S), 42, t + "c"), synth.normal((B, S, Eo), 42, t + "w")
    wo, wr = synth.normal((B, L, Eo), 42, t + "wo"), synth.normal((B, L, S), 42, t + "wr")
    kpm = mask_for(B, S) if S > 1 else None
    r32, r64 = (core_formula(x_sf.transpose(0, 1), u, c, w, kpm, wo, wr, dt) for dt in (torch.float32, torch.float64))
    xd = x_sf.to(cuda).requires_grad_()
    ud, cd, wd = (a.to(cuda).requires_grad_() for a in (u, c, w))
    xt = xd.transpose(0, 1)
    assert Fh._rows(xt) is xt, "the transpose of a sequence-first tensor is read in place"
    out, raw = Fh.few_key_attention(xt, ud, cd, wd, key_padding_mask=kpm.to(cuda) if kpm is not None else None, splits=2)
    assert out.shape == (B, L, Eo) and raw.shape == (B, L, S)
    ((out * wo.to(cuda)).sum() + (finite(raw) * wr.to(cuda)).sum() * 1e-2).backward()
    assert xd.grad.is_contiguous() and xd.grad.shape == (L, B, Eq)
    res = {"out": out, "raw": finite(raw), "dx": xd.grad.transpose(0, 1), "du": ud.grad, "dc": cd.grad, "dw": wd.grad}
    for key in res:
        assert_calibrated(f"core {Eq}/{Eo} S {S} {key}", res[key], r32[key], r64[key])
    if kpm is not None:
        assert torch.equal(torch.isinf(raw).cpu(), kpm[:, None, :].expand(B, L, S))
        for key in ("du", "dc", "dw"):
            assert bool((res[key].cpu()[kpm] == 0).all()), f"{key} of a masked key is exactly 0"


def test_unsupported_sizes_raise_on_device_tensors(cuda):
    z = lambda *s: torch.zeros(*s, device=cuda)          # noqa: E731
    with pytest.raises(ValueError, match="between 1 and 8 keys"):
        Fh.few_key_attention(z(2, 5, 256), z(2, 9, 256), z(2, 9), z(2, 9, 256))
    with pytest.raises(ValueError, match="multiples of 64"):
        Fh.few_key_attention(z(2, 5, 96), z(2, 4, 96), z(2, 4), z(2, 4, 256))
    mod = module(problem(3, 4, 11)[3], cuda)                        # the module does not raise: nine keys take the composed path
    out, raw = mod(z(5, 2, E), z(9, 2, E), z(9, 2, E))
    assert tuple(raw.shape) == (2, 1, 5, 9)


@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
def test_run_to_run_identity(cuda, det):
    for prob, splits in ((problem(3, 4, 300, "masked"), 7), (problem(3, 4, 300, "kv"), None)):
        a, b = hip_run(prob, cuda, splits=splits, det=det), hip_run(prob, cuda, splits=splits, det=det)
        for key in KEYS + ("masked",):
            if a[key] is not None:
                assert torch.equal(a[key], b[key]), f"{key} differs between two runs (deterministic: {det})"


def test_softmax_output(cuda):
    B, S, L = 3, 4, 300
    q, k, _, params, _, _, kpm = problem(B, S, L, "masked")
    r32, r64 = oracle(B, S, L, "masked")
    mod = module(params, cuda, splits=7)
    out, attn = mod(q.to(cuda), k.to(cuda), k.to(cuda), key_padding_mask=kpm.to(cuda), need_raw=False)
    assert tuple(attn.shape) == (B, L, S)
    assert_calibrated("softmax weights", attn, r32["softmax"], r64["softmax"])
    assert_close("softmax sums to one", attn.sum(-1), torch.ones(B, L))
    assert bool((attn.cpu()[kpm[:, None, :].expand(B, L, S)] == 0).all())
    assert mod(q.to(cuda), k.to(cuda), k.to(cuda), need_weights=False)[1] is None


def test_fused_against_composed(cuda):
    """The same module with fused_few_key off (two bag-sized projections, matmul4, softmax_rows, matmul4), same weights and inputs."""
    prob = problem(2, 4, 300)
    res, ref = hip_run(prob, cuda), hip_run(prob, cuda, fused=False)
    for key in KEYS:
        if ref[key] is not None:
            assert_close(f"fused vs composed {key}", res[key], ref[key])


@pytest.mark.parametrize("kw", [dict(bias=False), dict(kdim=64, vdim=128)], ids=["no in-projection bias", "kdim 64, vdim 128"])
def test_constructor_options_fused_against_composed(cuda, kw):
    """Options the oracle does not model: the same module with the flag on and off, same weights and inputs, ragged splits."""
    L, S, B = 37, 3, 2
    torch.manual_seed(4)
    mod = smml.MultiheadAttention(E, 1, **kw).to(cuda).eval()
    mod.fewk_splits = 2
    q = synth.normal((L, B, E), 42, "fewk_opts:q")
    k, v = synth.normal((S, B, mod.kdim), 42, "fewk_opts:k"), synth.normal((S, B, mod.vdim), 42, "fewk_opts:v")
    w_o, w_r = synth.normal((L, B, E), 42, "fewk_opts:wo").to(cuda), synth.normal((B, 1, L, S), 42, "fewk_opts:wr").to(cuda)
    runs = {}
    for on in (False, True):
        mod.fused_few_key = on
        mod.zero_grad()
        qd, kd, vd = (t.to(cuda).requires_grad_() for t in (q, k, v))
        out, raw = mod(qd, kd, vd)
        loss_of(out, raw, w_o, w_r).backward()
        runs[on] = {"out": out.detach(), "raw": raw.detach(), "dq": qd.grad, "dk": kd.grad, "dv": vd.grad}
        runs[on].update({"grad:" + n: p.grad.clone() for n, p in mod.named_parameters()})
    assert set(runs[True]) == set(runs[False])
    for key, ref in runs[False].items():
        assert_close(f"fused vs composed {key}", runs[True][key], ref)


@pytest.mark.parametrize("keys", [dict(coattn_fused_few_key=True), dict(coattn_fused=True, coattn_fused_few_key=True)],
                         ids=["few-key", "few-key and few-query"])
def test_cmta_golden_with_the_extension_key(cuda, keys):
    """CMTA at N = 150 with P_in_G_Att on the few-key kernels (and with both co-attention directions fused): the reference's fixture under
    the checks test_cmta_golden applies to the composed model."""
    from test_oracle_golden import CMTA_OUTPUTS, cmta_inputs, cmta_params
    g = Golden("cmta_n150")
    net = smml.CMTA(argparse.Namespace(label_dim=4, **keys))
    net.load_state_dict(cmta_params(net))
    net = net.to(cuda).eval()
    mod = net.P_in_G_Att
    assert mod.fused_few_key is True and net.G_in_P_Att.fused_few_query is bool(keys.get("coattn_fused"))
    assert Fh.coattn_few_key_why(S=len(net.omic_sizes), heads=mod.num_heads, Eq=mod.embed_dim, attn_mask=False, add_bias_kv=mod.bias_k is not None,
                                 add_zero_attn=mod.add_zero_attn, dropout_active=mod.training and mod.dropout > 0,
                                 fused=mod.fused_few_key) is None
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
