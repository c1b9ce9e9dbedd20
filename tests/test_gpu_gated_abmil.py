"""GPU: the gated attention pooling (mil.py GatedABMIL and ABMIL with `abmil_gated`, functional.attention_pool_gated, the gated kernels of
csrc/attn_pool.hip, the sigmoid and tanh | sigmoid epilogues of csrc/gemm.hip) against the reference's fixture and the fp64 oracle
tests/gated_abmil_oracle.py.  Every comparison goes through helpers.assert_calibrated / assert_zero_grad / assert_close / Golden.check
and lands in the parity report; the bounds are the suite's: 1e-4 of the tensor's scale, or 2 x the fp32 oracle's own distance from fp64.

Shapes: the forward kernel walks tiles of 16 rows inside each split of a bag; one row, 11 rows (less than one tile), 37 rows (three tiles
in one split), 300 rows cut into 7 splits of 43 (a ragged split of 42 whose last tile holds 10) or into 300 splits of one row, and 2501
rows with the library's own split count.  The score bias's gradient vanishes in exact arithmetic (softmax is shift invariant) and is held
to 1e-4 of sum |d s|."""
import functools

import pytest
import torch

import gated_abmil_oracle as go
from helpers import TOL, Golden, assert_calibrated, assert_close, assert_zero_grad, smml, synth
from test_abmil_host import net_args
from test_gated_abmil_host import check_against_fixture

pytestmark = pytest.mark.gpu
Fh = smml.functional
OUTPUTS = ("encoded", "logits", "softmax")
PEAKED_SEEDS = (42, 43, 44)          # one per bag; chosen so that the fp64 oracle alone meets the three conditions of test_peaked_softmax


@functools.lru_cache(maxsize=None)
def oracle(B, N, variant=""):
    """(problem, fp32 oracle, fp64 oracle) on the CPU, computed once per shape and shared, never modified."""
    prob = peaked_problem(B, N) if variant == "peaked" else go.problem(B, N)
    return prob, go.run(*prob, torch.float32), go.run(*prob, torch.float64)


@functools.lru_cache(maxsize=None)
def reference_oracle():
    prob = go.reference_problem(300)
    return prob, go.run_reference(*prob, torch.float32), go.run_reference(*prob, torch.float64)


def peaked_problem(B, N):
    """Scores spread over tens of units (attention_out.weight x 40) and two planted rows per bag: row N - 3 - in the last, ragged tile of the
    last split - scores 8 above every other row, row 5 - in the first tile - 5 above.  Planted by bisection on alpha v, where v is the
    least-squares solution of [Wv; Wu] v = [sign(w); 1]: alpha v drives every tanh unit towards sign(w) and every sigmoid unit towards 1,
    so its score grows with alpha."""
    assert B <= len(PEAKED_SEEDS)
    _, params, w_e, w_l = go.problem(B, N)
    x = torch.cat([go.problem(1, N, seed=sd)[0] for sd in PEAKED_SEEDS[:B]])
    params = {k: v.clone() for k, v in params.items()}
    params["attention_out.weight"] *= 40.0
    p = {k: v.double() for k, v in params.items()}
    wv, bv, wu, bu = p["attention_V.0.weight"], p["attention_V.0.bias"], p["attention_U.0.weight"], p["attention_U.0.bias"]
    w, b = p["attention_out.weight"][0], p["attention_out.bias"]
    score = lambda rows: (torch.tanh(rows @ wv.T + bv) * torch.sigmoid(rows @ wu.T + bu)) @ w + b          # noqa: E731
    v = torch.linalg.lstsq(torch.cat((wv, wu)), torch.cat((torch.sign(w), torch.ones_like(w)))[:, None]).solution[:, 0]
    for bag in range(B):
        top = float(score(x[bag].double()).max())
        for row, above in ((N - 3, 8.0), (5, 5.0)):
            lo, hi = 0.0, 8.0
            assert float(score((hi * v)[None])) > top + above
            for _ in range(60):
                mid = 0.5 * (lo + hi)
                lo, hi = (mid, hi) if float(score((mid * v)[None])) < top + above else (lo, mid)
            x[bag, row] = (hi * v).float()
    return x, params, w_e, w_l


def hip_run(prob, cuda, splits=None, det=False, shift=0.0):
    """The HIP module's evaluation of a problem in the layout of gated_abmil_oracle.run."""
    x, params, w_e, w_l = prob
    mod = smml.ABMIL(net_args(abmil_gated=True)).to(cuda)
    mod.load_state_dict(params, strict=True)
    mod.pool_splits = splits
    if shift:
        with torch.no_grad():
            mod.attention_out.bias += shift
    xc = x.to(cuda)
    with smml.deterministic(det):
        enc, logits, none = mod(xc)
    assert none is None
    loss = (enc * w_e.to(cuda)).sum() + (logits * w_l.to(cuda)).sum()
    loss.backward()
    res = {"encoded": enc.detach(), "logits": logits.detach(), "softmax": mod.attention_weights(xc), "loss": float(loss.detach())}
    res.update({"grad:" + k: v.grad.detach().clone() for k, v in mod.named_parameters()})
    torch.cuda.synchronize()
    return res


def check(name, res, r32, r64, outputs=OUTPUTS, params=go.NET_PARAMS, zero=go.NET_ZERO_GRAD):
    for k in tuple(outputs) + tuple("grad:" + p for p in params):
        if k == "grad:" + zero:
            assert_zero_grad(f"{name} d{zero}", res[k], r64["natural"])
        else:
            assert tuple(res[k].shape) == tuple(r64[k].shape), k
            assert_calibrated(f"{name} {k}", res[k], r32[k], r64[k])


def test_golden_parity(cuda):
    """The reference's own forward and loss through smml.GatedABMIL.forward."""
    g = Golden("gated_abmil_n300")
    (x, params, labels), r32, r64 = reference_oracle()
    mod = smml.GatedABMIL().to(cuda)
    mod.load_state_dict(params, strict=True)
    xc, lc = x.to(cuda), labels.to(cuda)
    prob, pred, labels_out, loss = mod(xc, lc, None, None)
    assert labels_out is lc and not prob.requires_grad and int(pred) == int(r64["prob"].argmax())
    loss.backward()
    res = {"prob": prob, "softmax": mod.attention_map(xc), "loss": float(loss.detach())}
    res.update({"grad:" + k: v.grad for k, v in mod.named_parameters()})
    assert tuple(res["softmax"].shape) == (1, 1, 300)
    check_against_fixture(g, res)           # the reference's fp32 values, the fixture's noise rule
    check("golden", res, r32, r64, outputs=("prob", "softmax"), params=go.PARAMS, zero=go.ZERO_GRAD)          # and the fp64 oracle
    assert abs(res["loss"] - r64["loss"]) <= TOL * abs(r64["loss"])
    assert_close("golden softmax sums to one", res["softmax"].sum(-1), torch.ones(1, 1))
    M = mod.pool(torch.cat((xc, xc)))          # the batched form
    assert tuple(M.shape) == (2, 1024) and torch.equal(M[0], M[1])


@pytest.mark.parametrize("B, N, splits", [(1, 1, None), (2, 11, None), (2, 37, None), (2, 37, 1), (3, 300, 1), (3, 300, 2), (3, 300, 7),
                                          (3, 300, 300), (1, 2501, None)])
def test_ragged_shapes(cuda, B, N, splits):
    prob, r32, r64 = oracle(B, N)
    check(f"ragged {B}x{N} splits {splits}", hip_run(prob, cuda, splits=splits), r32, r64)


def test_split_counts_agree(cuda):
    prob, _, _ = oracle(3, 300)
    runs = {s: hip_run(prob, cuda, splits=s) for s in (1, 2, 7)}
    for s in (2, 7):
        for k in OUTPUTS + tuple("grad:" + p for p in go.NET_PARAMS if p != go.NET_ZERO_GRAD):
            assert_close(f"splits {s} vs 1 {k}", runs[s][k], runs[1][k])


def test_peaked_softmax(cuda):
    prob, r32, r64 = oracle(3, 300, "peaked")
    A = r64["softmax"][:, 0]
    assert float(A[:, 297].min()) > 0.9 and float(A[:, 5].min()) > 0.01, "the planted rows carry the weight"
    s = torch.log(A)
    assert float((s.max(1).values - s.min(1).values).min()) > 35.0, "scores spread over tens of units"
    check("peaked", hip_run(prob, cuda, splits=7), r32, r64)
    check("peaked, library splits", hip_run(prob, cuda), r32, r64)


def test_shift_invariance(cuda):
    """attention_out.bias = +200: exp(s) overflows fp32 unless the max is subtracted; the outputs and gradients are those of bias + 0."""
    prob, r32, r64 = oracle(3, 300)
    check("bias +200", hip_run(prob, cuda, splits=7, shift=200.0), r32, r64)


def test_run_to_run_identity(cuda):
    prob, _, _ = oracle(3, 300)
    a = hip_run(prob, cuda, splits=7, det=True)
    b = hip_run(prob, cuda, splits=7, det=True)
    for k in OUTPUTS + tuple("grad:" + p for p in go.NET_PARAMS):
        assert torch.equal(a[k], b[k]), f"{k} differs between two deterministic runs"
    assert a["loss"] == b["loss"]


def test_differentiable_hidden_features(cuda):
    """attention_pool_gated without `hidden`: h2 is an ordinary input - its gradient (g hu | g hv) flows back through linear's own backward
    (the halves case of _Linear.backward) and gives the gradients the fused form gives."""
    prob, r32, r64 = oracle(2, 37)
    x, params, w_e, w_l = prob
    p = {k: v.to(cuda).requires_grad_() for k, v in params.items()}
    xc = x.to(cuda)
    h2 = Fh.linear(xc, torch.cat((p["attention_V.0.weight"], p["attention_U.0.weight"])),
                   torch.cat((p["attention_V.0.bias"], p["attention_U.0.bias"])), act=Fh.ACT_TANH_SIGMOID)
    sink = []
    M = Fh.attention_pool_gated(xc, h2, p["attention_out.weight"], p["attention_out.bias"], scores_out=sink)
    enc = Fh.linear(M, p["multimodal_projection.weight"], p["multimodal_projection.bias"])
    logits = Fh.linear(M, p["classifier.0.weight"], p["classifier.0.bias"])
    ((enc * w_e.to(cuda)).sum() + (logits * w_l.to(cuda)).sum()).backward()
    res = {"encoded": enc.detach(), "logits": logits.detach(), "softmax": torch.exp(sink[0] - sink[1][:, None])[:, None, :]}
    res.update({"grad:" + k: v.grad for k, v in p.items()})
    check("plain h2", res, r32, r64)


def test_input_gradient_is_refused(cuda):
    x, params, w_e, _ = oracle(2, 37)[0]
    mod = smml.ABMIL(net_args(abmil_gated=True)).to(cuda)
    enc, _, _ = mod(x.to(cuda).requires_grad_())
    with pytest.raises(RuntimeError, match="bag of features"):
        (enc * w_e.to(cuda)).sum().backward()


def _functional_case(D, dtype):
    """L = 256, N = 37, B = 2: a direct evaluation in `dtype` of M and of the gradients of (h2-free) Wv, bv, Wu, bu, w, b for
    loss = sum M g; 'natural' = sum |d s|."""
    B, N, L = 2, 37, 256
    tag = f"gated_fn{D}"
    x = synth.bag(B, N, L, 42, tag + ":bag").to(dtype)
    shapes = {"wv": (D, L), "bv": (D,), "wu": (D, L), "bu": (D,), "w": (1, D), "b": (1,)}
    p = {k: v.to(dtype).requires_grad_() for k, v in synth.fill_params(shapes, 42, tag).items()}
    g = synth.normal((B, L), 42, tag + ":g").to(dtype)
    s = (torch.tanh(x @ p["wv"].T + p["bv"]) * torch.sigmoid(x @ p["wu"].T + p["bu"])) @ p["w"].T + p["b"]
    natural = []
    s.register_hook(lambda gr: natural.append(float(gr.abs().sum())))
    M = torch.bmm(torch.softmax(s.transpose(2, 1), dim=2), x)[:, 0]
    (M * g).sum().backward()
    out = {"M": M.detach(), "natural": natural[0]}
    out.update({"grad:" + k: v.grad for k, v in p.items()})
    return (x, {k: v.detach() for k, v in p.items()}, g), out


@pytest.mark.parametrize("D", [64, 256])
def test_functional_form_at_other_hidden_widths(cuda, D):
    """One and four 64-column panels per half: both the fused (`hidden`) and the differentiable-h2 form against a direct fp64 evaluation."""
    (x, p, g), r32 = _functional_case(D, torch.float32)
    _, r64 = _functional_case(D, torch.float64)
    xc, gc = x.to(cuda), g.to(cuda)
    for fused in (True, False):
        q = {k: v.to(cuda).requires_grad_() for k, v in p.items()}
        wvu, bvu = torch.cat((q["wv"], q["wu"])), torch.cat((q["bv"], q["bu"]))
        if fused:
            with torch.no_grad():
                h2 = Fh.linear(xc, wvu, bvu, act=Fh.ACT_TANH_SIGMOID)
            M = Fh.attention_pool_gated(xc, h2, q["w"], q["b"], hidden=(q["wv"], q["bv"], q["wu"], q["bu"]))
        else:
            M = Fh.attention_pool_gated(xc, Fh.linear(xc, wvu, bvu, act=Fh.ACT_TANH_SIGMOID), q["w"], q["b"])
        (M * gc).sum().backward()
        name = f"functional D {D} {'fused' if fused else 'plain h2'}"
        assert_calibrated(f"{name} M", M, r32["M"], r64["M"])
        for k in ("wv", "bv", "wu", "bu", "w"):
            assert tuple(q[k].grad.shape) == tuple(r64["grad:" + k].shape)
            assert_calibrated(f"{name} d{k}", q[k].grad, r32["grad:" + k], r64["grad:" + k])
        assert_zero_grad(f"{name} db", q["b"].grad, r64["natural"])


def test_training_step(cuda):
    x = oracle(2, 300)[0][0].to(cuda)
    model = smml.define_net(net_args(mode="path", abmil_gated=True)).to(cuda)
    assert type(model) is smml.ABMIL and hasattr(model, "attention_out")
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    path_vec, logits, _ = model(x)                                  # as train_test.py:329 calls it
    loss = torch.nn.functional.cross_entropy(logits, torch.tensor([0, 2], device=cuda)) + 1e-3 * path_vec.pow(2).sum()
    opt.zero_grad()
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert tuple(path_vec.shape) == (2, 128) and tuple(logits.shape) == (2, 3) and bool(torch.isfinite(loss))
    for k, v in model.named_parameters():
        assert bool(torch.isfinite(v).all()), k
        if k != go.NET_ZERO_GRAD:                                   # its gradient is rounding noise around 0
            assert not torch.equal(v, before[k]), f"{k} did not move"


@pytest.mark.parametrize("act", ["sigmoid", "tanh_sigmoid"])
def test_gemm_epilogues(cuda, act):
    """linear 333 x 96 -> 128 with the sigmoid and the tanh | sigmoid epilogue: forward and the three gradients against fp64."""
    M, K, N = 333, 96, 128
    x = synth.normal((M, K), 42, "gated_epi:x")
    p = synth.fill_params({"w": (N, K), "b": (N,)}, 42, "gated_epi")
    g = synth.normal((M, N), 42, "gated_epi:g")
    xd, wd, bd = (t.double().requires_grad_() for t in (x, p["w"], p["b"]))
    pre = xd @ wd.T + bd
    y64 = torch.sigmoid(pre) if act == "sigmoid" else torch.cat((torch.tanh(pre[:, :N // 2]), torch.sigmoid(pre[:, N // 2:])), dim=1)
    (y64 * g.double()).sum().backward()
    xc, wc, bc = (t.to(cuda).requires_grad_() for t in (x, p["w"], p["b"]))
    y = Fh.linear(xc, wc, bc, act=Fh.ACT_SIGMOID if act == "sigmoid" else Fh.ACT_TANH_SIGMOID)
    (y * g.to(cuda)).sum().backward()
    assert_close(f"{act} y", y, y64, TOL)
    assert_close(f"{act} dx", xc.grad, xd.grad, TOL)
    assert_close(f"{act} dw", wc.grad, wd.grad, TOL)
    assert_close(f"{act} db", bc.grad, bd.grad, TOL)
