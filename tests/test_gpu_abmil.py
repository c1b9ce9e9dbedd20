"""GPU: ABMIL (mode 'path'; mil.py, functional.attention_pool, csrc/attn_pool.hip) against the reference's fixture and the fp64 oracle
tests/abmil_oracle.py.  Every comparison goes through helpers.assert_calibrated / assert_zero_grad / Golden.check and lands in the parity
report.  Bounds: the suite's floor of 1e-4 of the tensor's scale - the fp32 oracle's own gradients sit 2e-7 to 4e-6 from fp64 on the plain
problems (make_golden_abmil.py prints the reference's) and up to 3e-5 on the peaked one, so the noise term of the policy never exceeds
the floor.

Shapes: the forward kernel walks tiles of 16 rows inside each split of a bag; 11 rows are less than one tile, 37 rows three tiles in one
split, 300 rows cut into 7 splits of 43 end in a ragged split of 42 rows whose last tile holds 10, and 2501 rows take the library's own
split count.  d attention.2.bias vanishes in exact arithmetic (softmax is shift invariant) and is held to 1e-4 of sum |d s|."""
import functools

import pytest
import torch

import abmil_oracle as ao
from helpers import Golden, assert_calibrated, assert_close, assert_zero_grad, smml
from test_abmil_host import check_against_fixture, net_args

pytestmark = pytest.mark.gpu
Fh = smml.functional
OUTPUTS = ("encoded", "logits", "softmax")


@functools.lru_cache(maxsize=None)
def oracle(B, N, variant=""):
    """(problem, fp32 oracle, fp64 oracle) on the CPU, computed once per shape and shared, never modified."""
    prob = peaked_problem(B, N) if variant == "peaked" else ao.problem(B, N)
    return prob, ao.run(*prob, torch.float32), ao.run(*prob, torch.float64)


def peaked_problem(B, N):
    """Scores spread over tens of units (attention.2.weight x 40) and two planted rows per bag: row N - 3 - in the last, ragged tile of the
    last split - scores 8 above every other row, row 5 - in the first tile - 5 above.  The running max moves in the first tile and again in
    the last one, and the last split's partial outweighs the others in the merge."""
    x, params, w_e, w_l = ao.problem(B, N)
    params = {k: v.clone() for k, v in params.items()}
    params["attention.2.weight"] *= 40.0
    p = {k: v.double() for k, v in params.items()}
    w1, b1, w2, b2 = p["attention.0.weight"], p["attention.0.bias"], p["attention.2.weight"][0], p["attention.2.bias"]
    score = lambda rows: torch.tanh(rows @ w1.T + b1) @ w2 + b2          # noqa: E731
    v = torch.linalg.lstsq(w1, torch.sign(w2)[:, None]).solution[:, 0]   # w1 v = sign(w2): alpha v drives every hidden unit towards sign(w2)
    x = x.clone()
    for b in range(B):
        top = float(score(x[b].double()).max())
        for row, above in ((N - 3, 8.0), (5, 5.0)):
            lo, hi = 0.0, 8.0
            for _ in range(60):                                          # the score of alpha v grows with alpha: bisection
                mid = 0.5 * (lo + hi)
                lo, hi = (mid, hi) if float(score((mid * v)[None])) < top + above else (lo, mid)
            x[b, row] = (hi * v).float()
    return x, params, w_e, w_l


def hip_run(prob, cuda, splits=None, det=False, shift=0.0):
    """The HIP module's evaluation of a problem in the layout of abmil_oracle.run."""
    x, params, w_e, w_l = prob
    mod = smml.ABMIL(net_args()).to(cuda)
    mod.load_state_dict(params, strict=True)
    mod.pool_splits = splits
    if shift:
        with torch.no_grad():
            mod.attention[2].bias += shift
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


def check(name, res, r32, r64):
    for k in OUTPUTS + tuple("grad:" + p for p in ao.PARAMS):
        if k == "grad:" + ao.ZERO_GRAD:
            assert_zero_grad(f"{name} d{ao.ZERO_GRAD}", res[k], r64["natural"])
        else:
            assert tuple(res[k].shape) == tuple(r64[k].shape), k
            assert_calibrated(f"{name} {k}", res[k], r32[k], r64[k])


def test_golden_parity(cuda):
    g = Golden("abmil_n300")
    prob, r32, r64 = oracle(2, 300)
    res = hip_run(prob, cuda)
    assert tuple(res["softmax"].shape) == (2, 1, 300)
    check_against_fixture(g, res)           # the reference's fp32 values, the fixture's noise rule
    check("golden", res, r32, r64)          # and the fp64 oracle
    assert_close("golden softmax sums to one", res["softmax"].sum(-1), torch.ones(2, 1))


@pytest.mark.parametrize("B, N, splits", [(2, 11, None), (2, 37, None), (2, 37, 1), (3, 300, 1), (3, 300, 2), (3, 300, 7), (3, 300, 300),
                                          (1, 2501, None)])
def test_ragged_shapes(cuda, B, N, splits):
    prob, r32, r64 = oracle(B, N)
    check(f"ragged {B}x{N} splits {splits}", hip_run(prob, cuda, splits=splits), r32, r64)


def test_split_counts_agree(cuda):
    prob, _, _ = oracle(3, 300)
    runs = {s: hip_run(prob, cuda, splits=s) for s in (1, 2, 7)}
    for s in (2, 7):
        for k in OUTPUTS + tuple("grad:" + p for p in ao.PARAMS if p != ao.ZERO_GRAD):
            assert_close(f"splits {s} vs 1 {k}", runs[s][k], runs[1][k])


def test_peaked_softmax(cuda):
    prob, r32, r64 = oracle(3, 300, "peaked")
    A = r64["softmax"][:, 0]
    assert float(A[:, 297].min()) > 0.9 and float(A[:, 5].min()) > 0.01, "the planted rows carry the weight"
    s = torch.log(A)
    assert float((s.max(1).values - s.min(1).values).min()) > 40.0, "scores spread over tens of units"
    check("peaked", hip_run(prob, cuda, splits=7), r32, r64)
    check("peaked, library splits", hip_run(prob, cuda), r32, r64)


def test_shift_invariance(cuda):
    """attention.2.bias = +200: exp(s) overflows fp32 unless the max is subtracted; the outputs and gradients are those of bias + 0."""
    prob, r32, r64 = oracle(3, 300)
    check("bias +200", hip_run(prob, cuda, splits=7, shift=200.0), r32, r64)


def test_run_to_run_identity(cuda):
    prob, _, _ = oracle(3, 300)
    a = hip_run(prob, cuda, splits=7, det=True)
    b = hip_run(prob, cuda, splits=7, det=True)
    for k in OUTPUTS + tuple("grad:" + p for p in ao.PARAMS):
        assert torch.equal(a[k], b[k]), f"{k} differs between two deterministic runs"
    assert a["loss"] == b["loss"]


def test_differentiable_hidden_features(cuda):
    """attention_pool without `hidden`: h is an ordinary input - its gradient ds w2 flows back through linear's own backward and gives the
    gradients the fused form gives."""
    prob, r32, r64 = oracle(2, 37)
    x, params, w_e, w_l = prob
    p = {k: v.to(cuda).requires_grad_() for k, v in params.items()}
    xc = x.to(cuda)
    h = Fh.linear(xc, p["attention.0.weight"], p["attention.0.bias"], act=Fh.ACT_TANH)
    sink = []
    M = Fh.attention_pool(xc, h, p["attention.2.weight"], p["attention.2.bias"], scores_out=sink)
    enc = Fh.linear(M, p["multimodal_projection.weight"], p["multimodal_projection.bias"])
    logits = Fh.linear(M, p["classifier.0.weight"], p["classifier.0.bias"])
    ((enc * w_e.to(cuda)).sum() + (logits * w_l.to(cuda)).sum()).backward()
    res = {"encoded": enc.detach(), "logits": logits.detach(), "softmax": torch.exp(sink[0] - sink[1][:, None])[:, None, :]}
    res.update({"grad:" + k: v.grad for k, v in p.items()})
    check("plain h", res, r32, r64)


def test_input_gradient_is_refused(cuda):
    x, params, w_e, _ = oracle(2, 37)[0]
    mod = smml.ABMIL(net_args()).to(cuda)
    enc, _, _ = mod(x.to(cuda).requires_grad_())
    with pytest.raises(RuntimeError, match="bag of features"):
        (enc * w_e.to(cuda)).sum().backward()


def test_unsupported_width_raises_on_device_tensors(cuda):
    with pytest.raises(ValueError, match="feature width"):
        Fh.attention_pool(torch.zeros(1, 4, 768 + 128, device=cuda), torch.zeros(1, 4, 128, device=cuda), torch.zeros(1, 128, device=cuda),
                          torch.zeros(1, device=cuda))
    rc = smml.lib().smml_attn_pool_fwd_workspace_bytes(1, 4, 1024, 0)
    assert rc == 1 * 1 * (1024 + 4) * 4


def test_training_step(cuda):
    x = oracle(2, 300)[0][0].to(cuda)
    model = smml.define_net(net_args(mode="path")).to(cuda)
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
        if k != "attention.2.bias":                                 # its gradient is rounding noise around 0
            assert not torch.equal(v, before[k]), f"{k} did not move"
