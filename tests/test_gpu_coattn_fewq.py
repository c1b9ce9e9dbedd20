"""GPU: the few-query co-attention (MultiheadAttention.fused_few_query, functional.few_query_attention, csrc/fewq_attn.hip) against the
reference's fixture coattn_L4_S2500 and against oracle.coattn.coattention run on the CPU in fp32 and fp64.  Every comparison goes through
helpers.assert_calibrated / assert_close / Golden.check and lands in the parity report; no tolerance of its own.

Every loss carries the raw-score term of test_coattention_golden, (raw w_r).sum() 1e-2 over the finite entries: without it the key third of
in_proj_bias has no gradient (softmax is shift invariant).

Shapes: a workgroup walks tiles of 16 rows inside its split, four rows per wave.  11 rows are less than one tile, 37 rows three tiles in one
split, 300 rows cut into 7 splits of 43 end in a split of 42 rows whose last tile holds 10, 300 splits hold one row each; L = 1, 4 take the
four-query register layout, L = 6, 8 the eight-query one."""
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
    """bag 0: rows 43 .. 85, the whole of split 1 of 7; bag 1: row 0; bag 2: the last 7 rows"""
    kpm = torch.zeros(B, S, dtype=torch.bool)
    kpm[0, 43:86] = True; kpm[1, 0] = True; kpm[2, -7:] = True
    return kpm


@functools.lru_cache(maxsize=None)
def problem(B, L, S, variant=""):
    """(q [L, B, E], k [S, B, E], v or None (the values are the keys), params, w_o, w_r, key_padding_mask or None); never modified"""
    tag = f"fewq_{B}_{L}_{S}"
    params = params_for(smml.MultiheadAttention(E, 1), 42, tag)
    q, k = synth.normal((L, B, E), 42, tag + ":q"), synth.normal((S, B, E), 42, tag + ":kv")
    v = synth.normal((S, B, E), 42, tag + ":v") if variant == "kv" else None
    kpm = mask_for(B, S) if variant == "masked" else None
    if variant == "peaked":
        q, k = peaked(q, k, params)
    return q, k, v, params, synth.normal((L, B, E), 42, tag + ":wo"), synth.normal((B, 1, L, S), 42, tag + ":wr"), kpm


def peaked(q, k, params):
    """Queries scaled until every query's scores spread over 60 units, and two planted keys per bag along the direction every query scores
    positively: row 5 - in the first tile - 5 above every other key for the query that likes it least, row S - 3 - in the last, ragged tile
    of the last split - another 3 above that.  The running max moves in the first tile and again in the last one, and the last split's
    partial outweighs the others in the merge."""
    L, B, _ = q.shape
    S = k.shape[0]
    p = {n: t.double() for n, t in params.items()}
    w, b = p["in_proj_weight"], p["in_proj_bias"]
    score = lambda qq, kk: torch.einsum("lbe,sbe->bls", (qq.double() @ w[:E].t() + b[:E]) * E ** -0.5, kk.double() @ w[E:2 * E].t() + b[E:2 * E])  # noqa: E731
    r = score(q, k)
    q = q * float(60.0 / (r.max(-1).values - r.min(-1).values).min())
    k = k.clone()
    qh = (q.double() @ w[:E].t() + b[:E]) * E ** -0.5                                # [L, B, E]
    for bag in range(B):
        target = (qh[:, bag] / qh[:, bag].norm(dim=-1, keepdim=True)).sum(0)         # every query has a positive component along it
        v = torch.linalg.lstsq(w[E:2 * E], target[:, None]).solution[:, 0]           # Wk v = target
        gain = qh[:, bag] @ target
        assert float(gain.min()) > 0
        offs = qh[:, bag] @ b[E:2 * E]
        top = score(q, k)[bag].max(-1).values
        a5 = float(((top + 5.0 - offs) / gain).max())
        a_last = a5 + 3.0 / float(gain.min())
        k[5, bag] = (a5 * v).float()
        k[S - 3, bag] = (a_last * v).float()
    return q, k


def finite(raw):
    return torch.where(torch.isfinite(raw), raw, torch.zeros_like(raw))


def loss_of(out, raw, w_o, w_r):
    return (out * w_o).sum() + (finite(raw) * w_r).sum() * 1e-2


@functools.lru_cache(maxsize=None)
def oracle(B, L, S, variant=""):
    """(fp32, fp64) evaluations of oracle.coattn.coattention on the CPU, computed once per problem and shared"""
    q, k, v, params, w_o, w_r, kpm = problem(B, L, S, variant)
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
    mod.fused_few_query, mod.fewq_splits = fused, splits
    return mod.to(cuda).eval()


def hip_run(prob, cuda, splits=None, det=False, kv_grad=True):
    q, k, v, params, w_o, w_r, kpm = prob
    mod = module(params, cuda, splits)
    qd, kd = q.to(cuda).requires_grad_(), k.to(cuda).requires_grad_(kv_grad)
    vd = v.to(cuda).requires_grad_(kv_grad) if v is not None else kd
    with smml.deterministic(det):
        out, raw = mod(qd, kd, vd, key_padding_mask=kpm.to(cuda) if kpm is not None else None)
    assert tuple(out.shape) == tuple(q.shape) and tuple(raw.shape) == (q.shape[1], 1, q.shape[0], k.shape[0])
    loss_of(out, raw, w_o.to(cuda), w_r.to(cuda)).backward()
    torch.cuda.synchronize()
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
    tag, L, S, B = "coattn_L4_S2500", 4, 2500, 2
    g = Golden(tag)
    mod = module(params_for(smml.MultiheadAttention(E, 1), 42, tag), cuda)
    q = synth.normal((L, B, 256), 42, tag + ":q").to(cuda).requires_grad_()
    kv = synth.normal((S, B, 256), 42, tag + ":kv").to(cuda).requires_grad_()
    w_o = synth.normal((L, B, 256), 42, tag + ":wo").to(cuda); w_r = synth.normal((B, 1, L, S), 42, tag + ":wr").to(cuda)
    out, raw = mod(q, kv, kv)
    assert out.shape == (L, B, 256) and raw.shape == (B, 1, L, S)
    ((out * w_o).sum() + (raw * w_r).sum() * 1e-2).backward()
    g.check("out", out); g.check("raw", raw); g.check("dq", q.grad); g.check("dkv", kv.grad)
    for k, p in mod.named_parameters():
        g.check("grad:" + k, p.grad, what="d" + k)


@pytest.mark.parametrize("B, L, S, splits", [(2, 4, 11, None), (2, 1, 37, 1), (3, 4, 300, 1), (3, 4, 300, 7), (3, 8, 300, 7), (2, 6, 300, 300)])
def test_ragged_shapes(cuda, B, L, S, splits):
    check(f"ragged {B}x{L}x{S} splits {splits}", hip_run(problem(B, L, S), cuda, splits=splits), *oracle(B, L, S))


def test_split_counts_agree(cuda):
    runs = {s: hip_run(problem(3, 4, 300), cuda, splits=s) for s in (1, 2, 7)}
    for s in (2, 7):
        for key in KEYS:
            if runs[1][key] is not None:
                assert_close(f"splits {s} vs 1 {key}", runs[s][key], runs[1][key])


def test_key_padding_mask(cuda):
    B, L, S = 3, 4, 300
    prob, (r32, r64) = problem(B, L, S, "masked"), oracle(B, L, S, "masked")
    kpm = prob[6]
    res = hip_run(prob, cuda, splits=7)
    assert int(res["masked"].sum()) == int(r64["masked"].sum()) == L * (43 + 1 + 7)
    assert torch.equal(res["masked"].cpu(), kpm[:, None, None, :].expand(B, 1, L, S)), "raw is -inf exactly at the masked keys"
    rows = res["dk"].transpose(0, 1).cpu()[kpm]                     # [masked keys, E]
    assert rows.shape[0] == 51 and bool((rows == 0).all()), "gradient rows of masked keys are exactly 0"
    check("masked", res, r32, r64)
    check("masked, library splits", hip_run(prob, cuda), r32, r64)


def test_peaked_softmax(cuda):
    B, L, S = 3, 4, 300
    r32, r64 = oracle(B, L, S, "peaked")
    A, raw = r64["softmax"], r64["raw"][:, 0]
    assert float(A[:, :, S - 3].min()) > 0.9 and float(A[:, :, 5].max()) > 0.01, "the planted keys carry the weight"
    assert float((raw.max(-1).values - raw.min(-1).values).min()) > 40.0, "scores spread over tens of units"
    check("peaked", hip_run(problem(B, L, S, "peaked"), cuda, splits=7), r32, r64)
    check("peaked, library splits", hip_run(problem(B, L, S, "peaked"), cuda), r32, r64)


def test_distinct_key_and_value(cuda):
    B, L, S = 3, 4, 300
    r32, r64 = oracle(B, L, S, "kv")
    res = hip_run(problem(B, L, S, "kv"), cuda, splits=7)
    assert res["dv"] is not None and res["dk"].data_ptr() != res["dv"].data_ptr()
    check("key != value", res, r32, r64)


@pytest.mark.parametrize("variant", ["", "kv"])
def test_bag_without_gradient(cuda, variant):
    """Neither key nor value requires a gradient: no gradient row is formed, the parameter gradients are those of the full problem."""
    B, L, S = 3, 4, 300
    res = hip_run(problem(B, L, S, variant), cuda, splits=7, kv_grad=False)
    assert res["dk"] is None and res["dv"] is None
    check(f"no bag gradient {variant}", res, *oracle(B, L, S, variant), keys=("out", "raw", "dq") + tuple("grad:" + k for k in PARAMS))


def core_formula(u, c, x, y, wz, wr, wl, dt):
    u, c, x, y = (t.detach().clone().to(dt).requires_grad_() for t in (u, c, x, y))
    raw = u @ x.transpose(1, 2) + c[..., None]
    z, lse = torch.softmax(raw, -1) @ y, torch.logsumexp(raw, -1)
    ((z * wz.to(dt)).sum() + (raw * wr.to(dt)).sum() * 1e-2 + (lse * wl.to(dt)).sum()).backward()
    return {"z": z.detach(), "raw": raw.detach(), "lse": lse.detach(), "du": u.grad, "dc": c.grad, "dx": x.grad, "dy": y.grad}


def test_other_widths_through_the_functional(cuda):
    """Ek = 64, Ev = 128 (a quarter and a half of one 256-column panel), all three outputs in the loss, against the same formula on the CPU."""
    B, L, S, Ek, Ev = 2, 3, 37, 64, 128
    t = "fewq_widths:"
    u, c = synth.normal((B, L, Ek), 42, t + "u") * 0.3, synth.normal((B, L), 42, t + "c")
    x, y = synth.normal((B, S, Ek), 42, t + "x"), synth.normal((B, S, Ev), 42, t + "y")
    wz, wr, wl = synth.normal((B, L, Ev), 42, t + "wz"), synth.normal((B, L, S), 42, t + "wr"), synth.normal((B, L), 42, t + "wl")
    r32, r64 = core_formula(u, c, x, y, wz, wr, wl, torch.float32), core_formula(u, c, x, y, wz, wr, wl, torch.float64)
    ud, cd, xd, yd = (a.to(cuda).requires_grad_() for a in (u, c, x, y))
    z, raw, lse = Fh.few_query_attention(ud, cd, xd, yd, splits=2)
    ((z * wz.to(cuda)).sum() + (raw * wr.to(cuda)).sum() * 1e-2 + (lse * wl.to(cuda)).sum()).backward()
    res = {"z": z, "raw": raw, "lse": lse, "du": ud.grad, "dc": cd.grad, "dx": xd.grad, "dy": yd.grad}
    for key in res:
        assert_calibrated(f"widths 64/128 {key}", res[key], r32[key], r64[key])


def test_unsupported_sizes_raise_on_device_tensors(cuda):
    x = torch.zeros(2, 5, 256, device=cuda)
    with pytest.raises(ValueError, match="at most 8 queries"):
        Fh.few_query_attention(torch.zeros(2, 9, 256, device=cuda), torch.zeros(2, 9, device=cuda), x)
    with pytest.raises(ValueError, match="multiples of 64"):
        Fh.few_query_attention(torch.zeros(2, 4, 96, device=cuda), torch.zeros(2, 4, device=cuda), torch.zeros(2, 5, 96, device=cuda))
    mod = module(problem(2, 4, 11)[3], cuda)                        # the module does not raise: nine queries take the composed path
    out, raw = mod(torch.zeros(9, 2, E, device=cuda), x.transpose(0, 1), x.transpose(0, 1))
    assert tuple(raw.shape) == (2, 1, 9, 5)


def test_run_to_run_identity(cuda):
    prob = problem(3, 4, 300, "masked")
    a = hip_run(prob, cuda, splits=7, det=True)
    b = hip_run(prob, cuda, splits=7, det=True)
    for key in KEYS + ("masked",):
        if a[key] is not None:
            assert torch.equal(a[key], b[key]), f"{key} differs between two deterministic runs"


def test_softmax_output(cuda):
    B, L, S = 3, 4, 300
    q, k, _, params, _, _, kpm = problem(B, L, S, "masked")
    r32, r64 = oracle(B, L, S, "masked")
    mod = module(params, cuda, splits=7)
    out, attn = mod(q.to(cuda), k.to(cuda), k.to(cuda), key_padding_mask=kpm.to(cuda), need_raw=False)
    assert tuple(attn.shape) == (B, L, S)
    assert_calibrated("softmax weights", attn, r32["softmax"], r64["softmax"])
    assert_close("softmax sums to one", attn.sum(-1), torch.ones(B, L))
    assert bool((attn.cpu()[kpm[:, None, :].expand(B, L, S)] == 0).all())
    assert mod(q.to(cuda), k.to(cuda), k.to(cuda), need_weights=False)[1] is None


def test_cmta_with_the_extension_key(cuda):
    """CMTA at N = 150 with coattn_fused on and off, same weights: the seven outputs and every parameter gradient agree, and one Adam step
    leaves every parameter finite and moved."""
    from test_oracle_golden import CMTA_OUTPUTS, cmta_inputs, cmta_params
    x_path, x_omic, w = cmta_inputs()
    runs = {}
    for on in (False, True):
        net = smml.CMTA(argparse.Namespace(label_dim=4, coattn_fused=on))
        net.load_state_dict(cmta_params(net))
        net = net.to(cuda).eval()
        assert net.G_in_P_Att.fused_few_query is on
        out = net(x_path=x_path.to(cuda), x_omic=x_omic.to(cuda))
        loss = (out[0] * w[0].to(cuda)).sum() + sum((out[2 + i] * w[i].to(cuda)).sum() for i in range(1, 5))
        loss.backward()
        runs[on] = ([o.detach() for o in out], {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}, net)
    for nm, a, b in zip(CMTA_OUTPUTS, runs[True][0], runs[False][0]):
        assert_close("cmta fused vs composed " + nm, a, b)
    assert set(runs[True][1]) == set(runs[False][1])
    for k, gr in runs[True][1].items():
        assert_close("cmta fused vs composed d" + k, gr, runs[False][1][k])
    net = runs[True][2]
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    opt.step()
    torch.cuda.synchronize()
    for k, v in net.named_parameters():
        assert bool(torch.isfinite(v).all()), k
        if k in runs[True][1]:
            assert not torch.equal(v, before[k]), f"{k} did not move"


@pytest.mark.parametrize("kw", [dict(bias=False), dict(kdim=64, vdim=128)], ids=["no in-projection bias", "kdim 64, vdim 128"])
def test_constructor_options_fused_against_composed(cuda, kw):
    """Options the oracle does not model: the same module with the flag on and off, same weights and inputs, ragged splits."""
    L, S, B = 3, 37, 2
    torch.manual_seed(4)
    mod = smml.MultiheadAttention(E, 1, **kw).to(cuda).eval()
    mod.fewq_splits = 2
    q = synth.normal((L, B, E), 42, "fewq_opts:q")
    k, v = synth.normal((S, B, mod.kdim), 42, "fewq_opts:k"), synth.normal((S, B, mod.vdim), 42, "fewq_opts:v")
    w_o, w_r = synth.normal((L, B, E), 42, "fewq_opts:wo").to(cuda), synth.normal((B, 1, L, S), 42, "fewq_opts:wr").to(cuda)
    runs = {}
    for on in (False, True):
        mod.fused_few_query = on
        mod.zero_grad()
        qd, kd, vd = (t.to(cuda).requires_grad_() for t in (q, k, v))
        out, raw = mod(qd, kd, vd)
        loss_of(out, raw, w_o, w_r).backward()
        runs[on] = {"out": out.detach(), "raw": raw.detach(), "dq": qd.grad, "dk": kd.grad, "dv": vd.grad}
        runs[on].update({"grad:" + n: p.grad.clone() for n, p in mod.named_parameters()})
    assert set(runs[True]) == set(runs[False])
    for key, ref in runs[False].items():
        assert_close(f"fused vs composed {key}", runs[True][key], ref)


@pytest.mark.parametrize("detached", ["value", "key"])
def test_detached_alias_gets_no_share_of_the_gradient(cuda, detached):
    """`mod(q, kv, kv.detach())` (and the mirror image): key and value share memory, but only one side requires a gradient - it receives its
    own part alone, not the one-row sum dx + dy of the values-are-the-keys form.  Flag on against flag off, same weights and inputs."""
    B, L, S = 3, 4, 300
    q, k, _, params, w_o, w_r, _ = problem(B, L, S)
    runs = {}
    for on in (False, True):
        mod = module(params, cuda, splits=7, fused=on)
        qd, kv = q.to(cuda).requires_grad_(), k.to(cuda).requires_grad_()
        out, raw = mod(qd, kv, kv.detach()) if detached == "value" else mod(qd, kv.detach(), kv)
        loss_of(out, raw, w_o.to(cuda), w_r.to(cuda)).backward()
        runs[on] = {"out": out.detach(), "dq": qd.grad, "dkv": kv.grad}
        runs[on].update({"grad:" + n: p.grad for n, p in mod.named_parameters()})
    for key, ref in runs[False].items():
        assert_close(f"detached {detached}: fused vs composed {key}", runs[True][key], ref)
    whole = oracle(B, L, S)[1]["dk"]                         # the gradient of the shared tensor: the part must differ from it
    assert float((runs[True]["dkv"].cpu().double() - whole).abs().max()) > 1e-3 * float(whole.abs().max())
