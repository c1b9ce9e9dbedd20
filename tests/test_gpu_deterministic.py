"""GPU tests of the deterministic mode (functional.deterministic): the four kernel families that replace float
atomics by a partial slab and a fixed-order sum - split-K / folded-batch GEMM, LayerNorm backward, column sums, sampler backward - and a
whole training step.  Every case
  * runs the operation TWICE from identical inputs under the switch and asserts torch.equal on every output and gradient;
  * compares with an fp64 evaluation on the CPU at the suite's TOL (1e-4 of the tensor's scale; helpers.assert_close);
  * compares with the default mode at the same bound (the same sums in another order);
  * where noted copies one item into several batch slots and asserts bit-identical results in every slot: a fixed order is a function
    of the item's data alone.
The forward runs inside the `with` block and the backward after it has ended: the choice travels on the autograd context."""
import pytest
import torch

from helpers import TOL, assert_close, params_for, smml
from test_oracle_golden import pathomic_args

pytestmark = pytest.mark.gpu
Fh = smml.functional


@pytest.fixture(autouse=True)
def _switch_off():
    prev = Fh.is_deterministic()
    Fh.set_deterministic(False)
    yield
    Fh.set_deterministic(prev)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _run(fn, inputs, grad_outs, det):
    """fn(*leaves) -> tensor or tuple, forward under the switch `det`, backward AFTER the block -> (outputs, gradients of the leaves that
    require one), all detached clones."""
    leaves = [t.detach().clone().requires_grad_(t.requires_grad) for t in inputs]
    with smml.deterministic(det):
        out = fn(*leaves)
    outs = out if isinstance(out, tuple) else (out,)
    assert not Fh.is_deterministic()
    torch.autograd.backward(outs, [g.to(o.device) for g, o in zip(grad_outs, outs)])
    torch.cuda.synchronize()
    return [o.detach().clone() for o in outs], [l.grad.detach().clone() for l in leaves if l.requires_grad]


def _check(name, fn, inputs, grad_outs, ref_outs, ref_grads, out_names, grad_names):
    """The three comparisons every case makes; returns the deterministic run's (outputs, gradients) and the default run's."""
    a = _run(fn, inputs, grad_outs, True)
    b = _run(fn, inputs, grad_outs, True)
    d = _run(fn, inputs, grad_outs, False)
    for kind, names, refs, i in (("", out_names, ref_outs, 0), ("d ", grad_names, ref_grads, 1)):
        assert len(a[i]) == len(names) == len(refs)
        for n, x, y, z, r in zip(names, a[i], b[i], d[i], refs):
            assert torch.equal(x, y), f"{name}: {kind}{n} differs between two deterministic runs"
            assert_close(f"{name} {kind}{n} vs fp64", x, r)
            assert_close(f"{name} {kind}{n} vs default mode", x, z)
    return a, d


# ------------------------------------------------------------------------------------------------ 1. sampler backward
def _pixel_to_norm(ix, size):
    return (2.0 * ix + 1.0) / size - 1.0


def _hard_positions(G, J, Hh, Ww, gen):
    """vs [G, J, 2] (x, y): 20 points inside ONE pixel cell (long runs on four pixels), points on pixel centres (weights 0 / 1), points
    outside [-1, 1] on each side (masked corners), the rest uniform."""
    vs = torch.rand(G, J, 2, generator=gen) * 2 - 1
    cell = torch.rand(G, 20, 2, generator=gen) * 0.98 + 0.01                 # fractional position inside the cell (4, 7)
    vs[:, :20, 0] = _pixel_to_norm(4.0 + cell[..., 0], Ww)
    vs[:, :20, 1] = _pixel_to_norm(7.0 + cell[..., 1], Hh)
    centres = torch.tensor([[0.0, 0.0], [_pixel_to_norm(3.0, Ww), 0.0], [0.0, _pixel_to_norm(9.0, Hh)],
                            [_pixel_to_norm(0.0, Ww), _pixel_to_norm(0.0, Hh)], [_pixel_to_norm(Ww - 1.0, Ww), _pixel_to_norm(5.0, Hh)]])
    vs[:, 20:25] = centres
    outside = torch.tensor([[-1.3, 0.2], [1.25, -0.4], [0.1, -1.5], [0.3, 1.4], [-1.04, -1.04], [1.02, 0.99], [-2.5, 2.5]])
    vs[:, 25:32] = outside
    return vs.float()


def _sample_ref64(x, vs, cx0, cy0, G):
    """fp64 bilinear sampling (zeros outside, align_corners False) on the CELLS the kernels chose (cx0, cy0 = floor of the pixel
    coordinates as smml_bilinear_corners_f32 reports them): at a cell boundary two evaluations may floor differently, and d vs jumps there."""
    B, Hh, Ww, C = x.shape
    BG, J, PD = vs.shape
    cg = C // G
    ix = ((vs[..., 0] + 1) * Ww - 1) / 2
    iy = ((vs[..., 1] + 1) * Hh - 1) / 2 if PD == 2 else torch.full_like(ix, (Hh - 1) / 2)
    fx, fy = ix - cx0, iy - cy0
    xg = x.view(B, Hh * Ww, G, cg).permute(0, 2, 1, 3).reshape(BG, Hh * Ww, cg)
    out = 0
    for oy, ox in ((0, 0), (0, 1), (1, 0), (1, 1)):
        xx, yy = cx0 + ox, cy0 + oy
        m = (xx >= 0) & (xx < Ww) & (yy >= 0) & (yy < Hh)
        idx = yy.clamp(0, Hh - 1) * Ww + xx.clamp(0, Ww - 1)
        val = torch.gather(xg, 1, idx[..., None].expand(-1, -1, cg)) * m[..., None]
        out = out + val * ((fx if ox else 1 - fx) * (fy if oy else 1 - fy))[..., None]
    return out.view(B, G, J, cg).permute(0, 2, 1, 3).reshape(B, J, C)


def _sampler_case(cuda, name, B, Hh, Ww, G, cg, J, PD, vs_g):
    gen = _gen(3)
    C = G * cg
    x1 = torch.randn(1, Hh, Ww, C, generator=gen)
    dkv1 = torch.randn(1, J, C, generator=gen)
    x, dkv = x1.repeat(B, 1, 1, 1), dkv1.repeat(B, 1, 1)                      # ONE bag in every batch slot
    vs = vs_g.repeat(B, 1, 1)                                                # [(B G), J, PD], (b g)-major
    cx, cy, _ = Fh.bilinear_corners(vs.to(cuda), Hh, Ww, PD)
    cx0, cy0 = cx[:, 0].reshape(B * G, J).long().cpu(), cy[:, 0].reshape(B * G, J).long().cpu()
    x64, vs64 = x.double().requires_grad_(), vs.double().requires_grad_()
    kv64 = _sample_ref64(x64, vs64, cx0, cy0, G)
    kv64.backward(dkv.double())
    fn = lambda xx, vv: Fh.bilinear_sample(xx, vv, groups=G, posdim=PD)
    inputs = [x.to(cuda).requires_grad_(), vs.to(cuda).requires_grad_()]
    a, d = _check(name, fn, inputs, [dkv], [kv64.detach()], [x64.grad, vs64.grad], ["kv"], ["x", "vs"])
    dx, dvs = a[1]
    assert torch.equal(dvs, d[1][1]), f"{name}: d vs must be the default kernel's, bit for bit"
    for b in range(1, B):
        assert torch.equal(dx[b], dx[0]), f"{name}: d x of batch slot {b} differs from slot 0 (same bag)"
    return dx


@pytest.mark.parametrize("cg", [16, 32])
def test_sampler_backward_2d(cuda, cg):
    G, J, Hh, Ww = 4, 37, 13, 13
    vs_g = _hard_positions(G, J, Hh, Ww, _gen(11))
    dx = _sampler_case(cuda, f"sampler2d cg={cg}", 3, Hh, Ww, G, cg, J, 2, vs_g)
    # the long runs exist: the four pixels around cell (4, 7) collect 20 keys each, and a pixel nobody samples is exactly 0
    assert float(dx[0, 7, 4].abs().max()) > 0 and float(dx[0, 8, 5].abs().max()) > 0
    assert int((dx[0].abs().sum(-1) == 0).sum()) > 0


def test_sampler_backward_1d_degenerate_axis(cuda):
    """The 1-D module's layout: posdim 1 on a [Hh = 1, Ww = n] map; here every key of a group sits between the same two pixels (SURVEY K14:
    the reference's degenerate axis puts all J contributions on one pixel) plus a few spread ones."""
    G, J, Ww = 4, 25, 101
    gen = _gen(12)
    vs_g = torch.empty(G, J, 1)
    vs_g[:, :20, 0] = _pixel_to_norm(50.0 + torch.rand(G, 20, generator=gen) * 0.9, Ww)
    vs_g[:, 20, 0] = 0.0                                                      # pixel centre
    vs_g[:, 21, 0] = -1.2
    vs_g[:, 22, 0] = 1.3
    vs_g[:, 23:, 0] = torch.rand(G, 2, generator=gen) * 2 - 1
    _sampler_case(cuda, "sampler1d", 3, 1, Ww, G, 32, J, 1, vs_g.float())


def test_sampler_backward_rejects_more_than_4096_keys(cuda):
    gen = _gen(13)
    x = torch.randn(1, 4, 4, 16, generator=gen).to(cuda).requires_grad_()
    vs = (torch.rand(1, 4097, 2, generator=gen) * 2 - 1).to(cuda)
    with smml.deterministic():
        kv = Fh.bilinear_sample(x, vs, groups=1, posdim=2)
    with pytest.raises(RuntimeError, match="4096"):
        kv.sum().backward()
    kv = Fh.bilinear_sample(x, vs, groups=1, posdim=2)                        # the default mode has no such limit
    kv.sum().backward()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. LayerNorm backward
def _ln_ref(x, g, b, dy, token_mean):
    x64, g64, b64 = (t.double().requires_grad_() for t in (x, g, b))
    y = torch.nn.functional.layer_norm(x64, (x.shape[-1],), g64, b64, 1e-5)
    if token_mean:
        y = y.mean(dim=1)
    y.backward(dy.double())
    return y.detach(), [x64.grad, g64.grad, b64.grad]


@pytest.mark.parametrize("shape, token_mean", [((1003, 128), False), ((1003, 96), False), ((1003, 512), False), ((3, 335, 128), True)])
def test_layernorm_backward(cuda, shape, token_mean):
    gen = _gen(21)
    C = shape[-1]
    x = torch.randn(*shape, generator=gen) * 1.5 + 0.3
    g, b = torch.randn(C, generator=gen) * 0.5 + 1.0, torch.randn(C, generator=gen) * 0.2
    dy = torch.randn(*((shape[0], C) if token_mean else shape), generator=gen)
    y64, grads64 = _ln_ref(x, g, b, dy, token_mean)
    fn = (lambda xx, gg, bb: Fh.layer_norm_token_mean(xx, gg, bb)) if token_mean else (lambda xx, gg, bb: Fh.layer_norm(xx, gg, bb))
    inputs = [t.to(cuda).requires_grad_() for t in (x, g, b)]
    a, d = _check(f"layernorm {shape}", fn, inputs, [dy], [y64], grads64, ["y"], ["x", "gamma", "beta"])
    assert torch.equal(a[1][0], d[1][0]), "d x must be the default mode's, bit for bit"
    assert torch.equal(a[0][0], d[0][0]) or token_mean, "the forward is the default mode's (the token mean is a column sum)"


@pytest.mark.parametrize("C", [128, 96])
def test_layernorm_backward_adds_into_dgamma_dbeta(cuda, C):
    """The raw entry point keeps the accumulate-into contract (the shared LayerNorm of the two streams adds twice): non-zero buffers
    receive exactly buffer + sum."""
    L, capi = smml.lib(), smml._capi
    gen = _gen(22)
    R = 1003
    x = (torch.randn(R, C, generator=gen) * 1.5).to(cuda)
    dy = torch.randn(R, C, generator=gen).to(cuda)
    g, b = (torch.randn(C, generator=gen) * 0.5 + 1.0).to(cuda), torch.zeros(C, device=cuda)
    y, mean, rstd = torch.empty_like(x), torch.empty(R, device=cuda), torch.empty(R, device=cuda)
    capi.check(L.smml_layernorm_fwd_f32(capi.fptr(x), capi.fptr(g), capi.fptr(b), capi.fptr(y), capi.fptr(mean), capi.fptr(rstd), R, C, 1e-5,
                                        capi.stream()))
    wsb = L.smml_layernorm_bwd_det_workspace_bytes(R, C)
    res = []
    for fill in (0.0, 0.75):
        dx, dg, db = torch.empty_like(x), torch.full((C,), fill, device=cuda), torch.full((C,), -fill, device=cuda)
        ws = torch.empty(wsb // 4, device=cuda)
        capi.check(L.smml_layernorm_bwd_det_f32(capi.fptr(x), capi.fptr(dy), capi.fptr(g), capi.fptr(mean), capi.fptr(rstd), capi.fptr(dx),
                                                capi.fptr(dg), capi.fptr(db), R, C, 1, 1.0, 0, capi.fptr(ws), wsb, capi.stream()))
        torch.cuda.synchronize()
        res.append((dx, dg, db))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[1][1], res[0][1] + 0.75) and torch.equal(res[1][2], res[0][2] - 0.75)
    _, g64 = _ln_ref(x.cpu(), g.cpu(), b.cpu(), dy.cpu(), False)
    assert_close(f"layernorm raw C={C} d gamma", res[0][1], g64[1])
    assert_close(f"layernorm raw C={C} d beta", res[0][2], g64[2])
    too_small = L.smml_layernorm_bwd_det_f32(capi.fptr(x), capi.fptr(dy), capi.fptr(g), capi.fptr(mean), capi.fptr(rstd), capi.fptr(dx),
                                             capi.fptr(dg), capi.fptr(db), R, C, 1, 1.0, 0, capi.fptr(ws), wsb - 4, capi.stream())
    assert too_small < 0 and b"workspace" in L.smml_last_error()


# ------------------------------------------------------------------------------------------------ 3. column sums
@pytest.mark.parametrize("shape, replicate", [((3, 1001, 128), True), ((1, 777, 75), False), ((2, 5, 512), False)])
def test_column_sums(cuda, shape, replicate):
    gen = _gen(31)
    x = torch.randn(*shape, generator=gen)
    if replicate:
        x = x[:1].repeat(shape[0], 1, 1)
    ref = (x.double().sum(dim=1) * 0.37)
    xc = x.to(cuda)
    runs = []
    for det in (True, True, False):
        with smml.deterministic(det):
            runs.append(Fh.colsum(xc, 0.37))
        torch.cuda.synchronize()
    assert torch.equal(runs[0], runs[1])
    assert_close(f"colsum {shape} vs fp64", runs[0], ref)
    assert_close(f"colsum {shape} vs default mode", runs[0], runs[2])
    if replicate:
        for b in range(1, shape[0]):
            assert torch.equal(runs[0][b], runs[0][0]), f"batch slot {b} differs from slot 0 (same item)"


# ------------------------------------------------------------------------------------------------ 4. GEMM
def test_gemm_linear_backward_split_k(cuda):
    gen = _gen(41)
    M, K, N = 5000, 96, 40
    x, w, b = torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen) * 0.1, torch.randn(N, generator=gen)
    dy = torch.randn(M, N, generator=gen)
    assert Fh._splitk_for(N, K, M) > 1
    x64, w64, b64 = (t.double().requires_grad_() for t in (x, w, b))
    y64 = x64 @ w64.T + b64
    y64.backward(dy.double())
    inputs = [t.to(cuda).requires_grad_() for t in (x, w, b)]
    _check("linear 5000x96->40", lambda xx, ww, bb: Fh.linear(xx, ww, bb), inputs, [dy], [y64.detach()], [x64.grad, w64.grad, b64.grad], ["y"],
           ["x", "w", "b"])


def test_gemm_dual_linear_relu_backward(cuda):
    gen = _gen(42)
    M, K, N = 3000, 64, 128
    x = torch.randn(M, K, generator=gen)
    ws = [torch.randn(N, K, generator=gen) * 0.1 for _ in range(2)]
    bs = [torch.randn(N, generator=gen) * 0.1 for _ in range(2)]
    dys = [torch.randn(M, N, generator=gen) for _ in range(2)]
    assert Fh._splitk_for(N, K, M, 2) > 1
    inputs = [x.to(cuda), ws[0].to(cuda).requires_grad_(), bs[0].to(cuda).requires_grad_(), ws[1].to(cuda).requires_grad_(),
              bs[1].to(cuda).requires_grad_()]
    # the fp64 gradients on the ReLU decisions the kernel took (a pre-activation within rounding of 0 may fall either way in fp64)
    with torch.no_grad():
        y_hip = Fh.dual_linear_relu(*inputs)
    ref_out, ref_grads = [], []
    for i in range(2):
        pre = x.double() @ ws[i].double().T + bs[i].double()
        keep = (y_hip[i].cpu() > 0)
        ref_out.append(pre * keep)
        dpre = dys[i].double() * keep
        ref_grads += [dpre.T @ x.double(), dpre.sum(0)]
    _check("dual_linear_relu 3000x64->128", lambda *t: Fh.dual_linear_relu(*t), inputs, dys, ref_out, ref_grads, ["y0", "y1"],
           ["w0", "b0", "w1", "b1"])


def test_gemm_gram_forward_value(cuda):
    gen = _gen(43)
    x = torch.randn(1, 4, 40000, generator=gen).repeat(2, 1, 1)             # both items equal: replication check on the forward VALUE
    dg = torch.randn(2, 4, 4, generator=gen)
    x64 = x.double().requires_grad_()
    g64 = x64 @ x64.transpose(1, 2)
    g64.backward(dg.double())
    a, _ = _check("gram [2, 4, 40000]", lambda xx: Fh.gram(xx), [x.to(cuda).requires_grad_()], [dg], [g64.detach()], [x64.grad], ["gram"], ["x"])
    assert torch.equal(a[0][0][0], a[0][0][1]), "the two equal items give different Gram matrices"


def test_gemm_matmul4_backward_folded_batch(cuda):
    gen = _gen(44)
    A, B = torch.randn(1, 1, 64, 300, generator=gen), torch.randn(2, 3, 300, 32, generator=gen)
    dC = torch.randn(2, 3, 64, 32, generator=gen)
    A64, B64 = A.double().requires_grad_(), B.double().requires_grad_()
    C64 = A64 @ B64
    C64.backward(dC.double())
    inputs = [A.to(cuda).requires_grad_(), B.to(cuda).requires_grad_()]
    _check("matmul4 broadcast A", lambda a, b: Fh.matmul4(a, b), inputs, [dC], [C64.detach()], [A64.grad, B64.grad], ["C"], ["A", "B"])


def test_gemm_grouped_pointwise_weight_gradient(cuda):
    gen = _gen(45)
    G, cin, cout, n = 8, 16, 64, 900
    x, w = torch.randn(1, n, G * cin, generator=gen), torch.randn(G * cout, cin, generator=gen) * 0.2
    dy = torch.randn(1, n, G * cout, generator=gen)
    assert Fh._splitk_for(cout, cin, n, G) > 1
    x64, w64 = x.double().requires_grad_(), w.double().requires_grad_()
    y64 = torch.cat([x64[..., g * cin:(g + 1) * cin] @ w64[g * cout:(g + 1) * cout].T for g in range(G)], dim=-1)
    y64.backward(dy.double())
    inputs = [x.to(cuda).requires_grad_(), w.to(cuda).requires_grad_()]
    _check("grouped 1x1 8 x (16 -> 64)", lambda xx, ww: Fh.grouped_pointwise(xx, ww, G), inputs, [dy], [y64.detach()], [x64.grad, w64.grad],
           ["y"], ["x", "w"])


# ------------------------------------------------------------------------------------------------ 5. whole step
def _net(attn_dim):
    # the model returns a vgrid - what BatchLoss compares - only with attn_dim = 2 (with attn_dim = 1 and return_vgrid it raises, as the
    # reference does): the 1-D step therefore runs without the two BatchLoss terms
    return smml.DeformPathomicNet(pathomic_args(input_path_dim=64, grid_hw=(20, 20), attn_dim=attn_dim, return_vgrid=attn_dim == 2,
                                                dropout_rate=0.1))


def _train_two_steps(cuda, attn_dim, det, state):
    net = _net(attn_dim)
    net.load_state_dict(state)
    net = net.to(cuda).train()
    B = 2
    bl = smml.BatchLoss(B, 1)
    x_path = smml.synth.bag(B, 400, 64, 42, "det:bag").to(cuda)
    x_t, x_i = smml.synth.normal((B, 59), 42, "det:tumor").to(cuda), smml.synth.normal((B, 361), 42, "det:immune").to(cuda)
    label = torch.tensor([1, 3], device=cuda)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    torch.manual_seed(0)
    losses, first_grads = [], None
    with smml.deterministic(det):
        for step in range(2):
            opt.zero_grad(set_to_none=True)
            feats, _, _, lg = net(x_path=x_path, x_omic=None, x_omic_tumor=x_t, x_omic_immune=x_i)[:4]
            loss = torch.nn.functional.cross_entropy(lg[2], label)
            if attn_dim == 2:
                loss = loss + 0.5 * bl(lg[3], lg[4]).sum() + 0.5 * bl(lg[5], lg[6]).sum()
            else:                                      # the loss of test_region1d_pathomic_step_key_true_vs_false
                loss = loss + feats.pow(2).mean()
            loss.backward()
            if step == 0:
                first_grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
            opt.step()
            losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    return losses, first_grads, {k: p.detach().clone() for k, p in net.named_parameters()}


@pytest.mark.parametrize("attn_dim", [2, 1])
def test_training_step_is_run_to_run_identical(cuda, attn_dim):
    """Two Adam steps of DeformPathomicNet (train mode, dropout 0.1) + cross-entropy + 0.5 x both BatchLoss sums (attn_dim 2; attn_dim 1
    has no vgrid to feed BatchLoss and takes cross-entropy + mean(feats^2)), twice from one state_dict and torch.manual_seed(0): both
    losses and every parameter after the second step bit-equal; the default mode's first-step gradients within the bound of
    test_region1d_pathomic_step_key_true_vs_false (5e-4 of each gradient's scale, loss 2e-5)."""
    proto = _net(attn_dim)
    state = params_for(proto, 42, "pathomic")
    la, ga, pa = _train_two_steps(cuda, attn_dim, True, state)
    lb, gb, pb = _train_two_steps(cuda, attn_dim, True, state)
    for s in range(2):
        assert torch.equal(la[s], lb[s]), f"loss of step {s}: {float(la[s])!r} vs {float(lb[s])!r}"
    assert ga.keys() == gb.keys() and pa.keys() == pb.keys()
    bad = [k for k in ga if not torch.equal(ga[k], gb[k])]
    assert not bad, f"first-step gradients differ between two deterministic runs: {bad}"
    bad = [k for k in pa if not torch.equal(pa[k], pb[k])]
    assert not bad, f"parameters after the second step differ between two deterministic runs: {bad}"
    ld, gd, _ = _train_two_steps(cuda, attn_dim, False, state)
    print(f"attn_dim={attn_dim}: loss deterministic {float(la[0])!r} default {float(ld[0])!r}")
    assert abs(float(la[0]) - float(ld[0])) <= 2e-5 * max(abs(float(ld[0])), 1e-30)
    assert ga.keys() == gd.keys()
    for k, g0 in gd.items():
        scale = float(g0.abs().max())
        if scale < 1e-12 or k.endswith("rel_pos_bias.mlp.2.bias"):            # d b3: the sum of all d scores, zero in exact arithmetic
            continue
        err = float((ga[k] - g0).abs().max()) / scale
        assert err <= 5e-4, f"d{k}: deterministic vs default mode differ by {err:.2e} of its scale"


# ------------------------------------------------------------------------------------------------ 6. uncovered paths raise
def test_nystrom_translayer_backward_raises(cuda):
    tl = smml.TransLayer(dim=64)
    tl.load_state_dict(params_for(tl, 42, "translayer"))
    tl = tl.to(cuda).eval()
    x = smml.synth.normal((2, 37, 64), 42, "translayer:x").to(cuda).requires_grad_()
    with smml.deterministic():
        out = tl(x)
    with pytest.raises(RuntimeError, match="res_conv.*no deterministic form"):
        out.sum().backward()
    tl.zero_grad(set_to_none=True)
    tl(x).sum().backward()                                                    # the default mode is untouched
    torch.cuda.synchronize()


def test_linear_b16_backward_raises(cuda):
    gen = _gen(61)
    x = torch.randn(100, 64, generator=gen).to(cuda).to(torch.bfloat16)
    w = (torch.randn(32, 64, generator=gen) * 0.1).to(cuda).requires_grad_()
    with smml.deterministic():
        y = Fh.linear_b16(x, w, None, out_bf16=False)
    with pytest.raises(RuntimeError, match="linear_b16.*no deterministic form"):
        y.sum().backward()
    assert w.grad is None
    Fh.linear_b16(x, w, None, out_bf16=False).sum().backward()
    torch.cuda.synchronize()
    assert w.grad is not None


# ------------------------------------------------------------------------------------------------ 7. hipGraph capture
def test_deterministic_ops_capture_in_a_graph(cuda):
    """No host synchronisation or data-dependent host decision enters the mode: the four families, forward and backward, are captured in
    a hipGraph (workspaces are torch.empty tensors of the graph's pool) and a replay reproduces the eager results bit for bit."""
    gen = _gen(71)
    G, cg, J, Hh, Ww = 4, 16, 37, 13, 13
    x = torch.randn(700, 96, generator=gen).to(cuda)
    w = (torch.randn(128, 96, generator=gen) * 0.1).to(cuda).requires_grad_()
    b = torch.randn(128, generator=gen).to(cuda).requires_grad_()
    gam, bet = torch.ones(128, device=cuda).requires_grad_(), torch.zeros(128, device=cuda).requires_grad_()
    img = torch.randn(2, Hh, Ww, G * cg, generator=gen).to(cuda).requires_grad_()
    vs = _hard_positions(G, J, Hh, Ww, _gen(72)).repeat(2, 1, 1).to(cuda)
    leaves = [w, b, gam, bet, img]

    def step():
        for t in leaves:
            t.grad = None
        with smml.deterministic():
            y = Fh.layer_norm(Fh.linear(x, w, b), gam, bet)                   # split-K dW, column-sum db, LayerNorm backward
            kv = Fh.bilinear_sample(img, vs, groups=G, posdim=2)              # sampler backward
            loss = Fh.token_mean(y.view(2, 350, 128)).pow(2).sum() + kv.pow(2).sum()
        loss.backward()
        return loss

    assert Fh._splitk_for(128, 96, 700) > 1
    loss_e = step().detach().clone()
    torch.cuda.synchronize()
    grads_e = [t.grad.detach().clone() for t in leaves]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                                                # warm-up on the capture stream
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            loss_g = step()
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss_g.detach(), loss_e)
    for t, ge in zip(leaves, grads_e):
        assert torch.equal(t.grad, ge)
