"""The row passes around the dense layers of the path, where the step no longer touches a [B, N, 128] tensor it does not need:

  * A  LayerNorm backward at C = 128: every tail of a trip (and of the eight-row trip that was tried), a ragged multi-workgroup end,
       broadcast gradient rows (rows_per_dy, dy_scale), accumulate_dx, the deterministic entry point;
  * B  functional.GradSum: the two gradients of a tensor that feeds a layer_norm and a linear (as residual, or as x) meet in one buffer -
       bit-equal to what autograd's add gives, in either order of the two producers;
  * C  the token mean of LayerNorm(x) without the normalised tensor (128 columns; other widths keep the composed route).

(D of the same plan, ReLU backward with the bias gradient in one pass, was measured slower than the two passes it replaced and is not built:
DESIGN.md section 5.)

Bound: the suite's default, 1e-4 of the tensor's scale (tests/helpers.py), against fp64 on the CPU; bit-equality where the arithmetic is the
same operation on the same operands."""
import importlib

import pytest
import torch
import torch.nn.functional as F

from helpers import assert_close, smml, synth

pytestmark = pytest.mark.gpu
Fh = smml.functional
capi = importlib.import_module("subspace-multimodal-learning_amd._capi")
EPS = 1e-5


# ------------------------------------------------------------------------------------------------
# A: LayerNorm backward
# ------------------------------------------------------------------------------------------------
def _ln_inputs(R, C, tag, dy_rows=None):
    x = synth.normal((R, C), 41, f"{tag}:x")
    g = synth.normal((C,), 41, f"{tag}:g", std=0.1, mean=1.0)
    b = synth.normal((C,), 41, f"{tag}:b", std=0.1)
    dy = synth.normal((dy_rows or R, C), 41, f"{tag}:dy")
    return x, g, b, dy


def _ln_stats(cuda, x, g, b):
    """x, gamma, beta on the device with the forward's saved mean / rstd"""
    R, C = x.shape
    xd, gd, bd = x.to(cuda), g.to(cuda), b.to(cuda)
    y, mu, rs = torch.empty_like(xd), torch.empty(R, device=cuda), torch.empty(R, device=cuda)
    capi.check(capi.lib().smml_layernorm_fwd_f32(capi.fptr(xd), capi.fptr(gd), capi.fptr(bd), capi.fptr(y), capi.fptr(mu), capi.fptr(rs),
                                                 R, C, EPS, capi.stream()), "layernorm_fwd")
    return xd, gd, bd, mu, rs


def _ln_bwd(cuda, xd, dyd, gd, mu, rs, rows_per_dy=1, dy_scale=1.0, into=None, det=False):
    R, C = xd.shape
    L = capi.lib()
    dx = torch.empty_like(xd) if into is None else into.clone()
    dg, db = torch.zeros(C, device=cuda), torch.zeros(C, device=cuda)
    args = (capi.fptr(xd), capi.fptr(dyd), capi.fptr(gd), capi.fptr(mu), capi.fptr(rs), capi.fptr(dx), capi.fptr(dg), capi.fptr(db), R, C,
            rows_per_dy, dy_scale, 0 if into is None else 1)
    if det:
        wsb = L.smml_layernorm_bwd_det_workspace_bytes(R, C)
        ws = torch.empty((wsb + 3) // 4, device=cuda)
        capi.check(L.smml_layernorm_bwd_det_f32(*args, capi.fptr(ws), wsb, capi.stream()), "layernorm_bwd_det")
    else:
        capi.check(L.smml_layernorm_bwd_f32(*args, capi.stream()), "layernorm_bwd")
    return dx, dg, db


@pytest.mark.parametrize("R", [1, 2, 7, 8, 9, 15, 16, 17, 33, 4099])
def test_layernorm_bwd128_row_tails(cuda, R):
    """C = 128: one row, a few, one wave's trip (8), one more, two waves' worth and one more, a second workgroup (33), 129 workgroups with a
    ragged end - dx, dgamma and dbeta against fp64"""
    C, tag = 128, f"lnb128:{R}"
    x, g, b, dy = _ln_inputs(R, C, tag)
    x64, g64, b64 = x.double().requires_grad_(), g.double().requires_grad_(), b.double().requires_grad_()
    (F.layer_norm(x64, (C,), g64, b64, EPS) * dy.double()).sum().backward()
    xd, gd, _, mu, rs = _ln_stats(cuda, x, g, b)
    dx, dg, db = _ln_bwd(cuda, xd, dy.to(cuda), gd, mu, rs)
    assert_close(f"{tag}:dx", dx, x64.grad)
    assert_close(f"{tag}:dgamma", dg, g64.grad)
    assert_close(f"{tag}:dbeta", db, b64.grad)


def test_layernorm_bwd128_broadcast_rows_and_scale(cuda):
    """rows_per_dy = n with a dy_scale: the gradient of 0.37 x the sum over each bag's tokens, R = 3 x 37"""
    nb, n, C, sc, tag = 3, 37, 128, 0.37, "lnb128:bcast"
    x, g, b, dy = _ln_inputs(nb * n, C, tag, dy_rows=nb)
    x64, g64, b64 = x.double().requires_grad_(), g.double().requires_grad_(), b.double().requires_grad_()
    y64 = F.layer_norm(x64, (C,), g64, b64, EPS).reshape(nb, n, C)
    (y64.sum(1) * sc * dy.double()).sum().backward()
    xd, gd, _, mu, rs = _ln_stats(cuda, x, g, b)
    dx, dg, db = _ln_bwd(cuda, xd, dy.to(cuda), gd, mu, rs, rows_per_dy=n, dy_scale=sc)
    assert_close(f"{tag}:dx", dx, x64.grad)
    assert_close(f"{tag}:dgamma", dg, g64.grad)
    assert_close(f"{tag}:dbeta", db, b64.grad)


@pytest.mark.parametrize("C", [128, 192])
def test_layernorm_bwd_accumulate_dx_is_a_separate_add(cuda, C):
    """accumulate_dx = 1 onto a random buffer = the accumulate_dx = 0 result + that buffer, rounded once: bit-equal (128: the fast kernel,
    ragged end; 192: the generic one)"""
    R, tag = 4099, f"lnb{C}:acc"
    x, g, b, dy = _ln_inputs(R, C, tag)
    xd, gd, _, mu, rs = _ln_stats(cuda, x, g, b)
    buf = synth.normal((R, C), 41, f"{tag}:buf").to(cuda)
    dx0, _, _ = _ln_bwd(cuda, xd, dy.to(cuda), gd, mu, rs)
    dx1, _, _ = _ln_bwd(cuda, xd, dy.to(cuda), gd, mu, rs, into=buf)
    assert torch.equal(dx1, dx0 + buf)


def test_layernorm_bwd128_deterministic_twice(cuda):
    """the deterministic entry point, twice on the same input: dx, dgamma, dbeta bit-equal; dx is the default entry point's"""
    R, C, tag = 4099, 128, "lnb128:det"
    x, g, b, dy = _ln_inputs(R, C, tag)
    xd, gd, _, mu, rs = _ln_stats(cuda, x, g, b)
    a = _ln_bwd(cuda, xd, dy.to(cuda), gd, mu, rs, det=True)
    c = _ln_bwd(cuda, xd, dy.to(cuda), gd, mu, rs, det=True)
    d = _ln_bwd(cuda, xd, dy.to(cuda), gd, mu, rs)
    for name, u, v in zip(("dx", "dgamma", "dbeta"), a, c):
        assert torch.equal(u, v), f"{tag}:{name} differs between two deterministic runs"
    assert torch.equal(a[0], d[0])
    assert_close(f"{tag}:dgamma vs default", a[1], d[1].double())


# ------------------------------------------------------------------------------------------------
# B: two gradients of one tensor in one buffer
# ------------------------------------------------------------------------------------------------
def _fork_params(C, tag):
    return {"g": synth.normal((C,), 42, f"{tag}:g", std=0.1, mean=1.0), "b": synth.normal((C,), 42, f"{tag}:b", std=0.1),
            "w": synth.normal((C, C), 42, f"{tag}:w", std=C ** -0.5), "wb": synth.normal((C,), 42, f"{tag}:wb", std=0.1)}


def _two_consumers(cuda, form, norm_first, fork, p, x, w1, w2):
    """x.grad of sum(w1 layer_norm(x)) + sum(w2 linear(...)) with x also the linear's residual (form 'residual': the fusion output h) or its
    input with a per-bag bias row (form 'x': the fusion layer over `path`).  Of two nodes that are ready together autograd runs the one
    made LAST first: norm_first makes the LayerNorm first, so that the linear's backward runs first and parks."""
    B, n, C = x.shape
    xd = x.to(cuda).requires_grad_()
    t = Fh.grad_sum(xd.view_as(xd)) if fork else xd.view_as(xd)
    g, b, w, wb = (p[k].to(cuda) for k in ("g", "b", "w", "wb"))

    def lin():
        if form == "residual":
            return Fh.linear(synth.normal((B, n, C), 43, "fork:o").to(cuda), w, wb, residual=t)
        return Fh.linear(t, w, synth.normal((B, C), 43, "fork:rowbias").to(cuda), rows_per_bias=n)

    def norm():
        return Fh.layer_norm(t, g, b, EPS)

    a, c = (norm(), lin()) if norm_first else tuple(reversed((lin(), norm())))
    ((a * w1.to(cuda)).sum() + (c * w2.to(cuda)).sum()).backward()
    return xd.grad


@pytest.mark.parametrize("norm_first", [True, False])
@pytest.mark.parametrize("form", ["residual", "x"])
def test_grad_sum_matches_autograd_add_bit_for_bit(cuda, form, norm_first):
    B, n, C = 2, 37, 128
    p = _fork_params(C, "fork")
    x = synth.normal((B, n, C), 42, "fork:x")
    w1, w2 = synth.normal((B, n, C), 42, "fork:w1"), synth.normal((B, n, C), 42, "fork:w2")
    assert Fh.GRAD_SUM
    plain = _two_consumers(cuda, form, norm_first, False, p, x, w1, w2)
    calls = []
    take = Fh.GradSum.take

    def spy(self, who, like):
        r = take(self, who, like)
        calls.append((who, r is not None))
        return r

    Fh.GradSum.take = spy
    try:
        joined = _two_consumers(cuda, form, norm_first, True, p, x, w1, w2)
    finally:
        Fh.GradSum.take = take
    assert torch.equal(joined, plain)
    # the order the test asked for was the order that ran: the second producer found the first one's gradient
    second = "norm" if norm_first else "linear"
    if form == "x":
        assert calls == [("linear" if norm_first else "norm", False), (second, True)], calls
    else:                                      # a residual's linear only parks: the LayerNorm adds (norm_first), or autograd does
        assert calls == [("norm", norm_first)], calls
    # fp64 truth of the sum
    x64 = x.double().requires_grad_()
    y1 = F.layer_norm(x64, (C,), p["g"].double(), p["b"].double(), EPS)
    y2 = x64 if form == "residual" else F.linear(x64, p["w"].double())
    ((y1 * w1.double()).sum() + (y2 * w2.double()).sum()).backward()
    assert_close(f"fork:{form}:{norm_first}:dx", joined, x64.grad)


def test_grad_sum_is_left_alone_by_partial_backward_passes(cuda):
    """two backward passes over one graph, one consumer each: a parked gradient is never taken by another pass"""
    B, n, C = 2, 37, 128
    p = _fork_params(C, "fork2")
    xd = synth.normal((B, n, C), 42, "fork2:x").to(cuda).requires_grad_()
    t = Fh.grad_sum(xd.view_as(xd))
    y1 = Fh.layer_norm(t, p["g"].to(cuda), p["b"].to(cuda), EPS)
    y2 = Fh.linear(t, p["w"].to(cuda))
    w1, w2 = synth.normal((B, n, C), 42, "fork2:w1").to(cuda), synth.normal((B, n, C), 42, "fork2:w2").to(cuda)
    g1, = torch.autograd.grad((y1 * w1).sum(), xd, retain_graph=True)
    keep = g1.clone()
    g2, = torch.autograd.grad((y2 * w2).sum(), xd)
    assert torch.equal(g1, keep)
    assert_close("fork2:dx of the linear", g2, (w2.double().cpu() @ p["w"].double()))


# ------------------------------------------------------------------------------------------------
# C: token mean of LayerNorm(x)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 37, 128), (3, 300, 128), (1, 1, 128), (2, 1100, 128), (2, 37, 64), (2, 37, 256)])
def test_layernorm_token_mean(cuda, shape):
    """128 columns: the fused kernel - bags of one chunk (37 and 300 rows: every tail of a trip; a single row) and, past 1024 tokens, of 18
    chunks of 64 rows with a ragged last one; its saved mean / rstd are the plain forward's bits.  64 and 256 columns: the composed route
    (the fused entry point refuses them), same checks."""
    B, n, C = shape
    tag = f"lntm:{B}x{n}x{C}"
    x = synth.normal(shape, 44, f"{tag}:x")
    g = synth.normal((C,), 44, f"{tag}:g", std=0.1, mean=1.0)
    b = synth.normal((C,), 44, f"{tag}:b", std=0.1)
    w = synth.normal((B, C), 44, f"{tag}:w")
    x64 = x.double().requires_grad_()
    m64 = F.layer_norm(x64, (C,), g.double(), b.double(), EPS).mean(1)
    (m64 * w.double()).sum().backward()
    xd, gd, bd = x.to(cuda).requires_grad_(), g.to(cuda), b.to(cuda)
    m = Fh.layer_norm_token_mean(xd, gd, bd, EPS)
    saved = m.grad_fn.saved_tensors
    (m * w.to(cuda)).sum().backward()
    assert_close(f"{tag}:mean", m, m64)
    assert_close(f"{tag}:dx", xd.grad, x64.grad)
    _, _, _, mu, rs = _ln_stats(cuda, x.reshape(B * n, C), g, b)
    assert torch.equal(saved[2], mu) and torch.equal(saved[3], rs)
    L = capi.lib()
    out = torch.zeros(B, C, device=cuda)
    rc = L.smml_layernorm_fwd_mean_f32(capi.fptr(xd.detach()), capi.fptr(gd), capi.fptr(bd), capi.fptr(mu), capi.fptr(rs), capi.fptr(out), B, n, C,
                                       EPS, capi.stream())
    assert (rc == 0) == (C == 128)
    if C == 128:
        assert_close(f"{tag}:mean through the C-ABI", out, m64)
        with smml.deterministic():
            runs = [Fh.layer_norm_token_mean(xd.detach(), gd, bd, EPS) for _ in range(2)]
        assert torch.equal(runs[0], runs[1])
        assert_close(f"{tag}:mean (deterministic)", runs[0], m64)
