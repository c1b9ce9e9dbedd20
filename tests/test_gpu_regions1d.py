"""GPU tests of the 1-D position bias per linear piece of its MLP (csrc/cpb_regions1d.h; include/smml.h "region1d" entry points).
The MLP of DeformableAttention1D.py:69-98 is piecewise affine in ONE signed-log offset.  These tests pin
  * the TABLES against an fp64 restatement of the breakpoints, patterns and (a, c) written here, and the kernels' lookup against fp64;
  * the KERNELS against the per-pair MLP kernels on the same inputs (the bounds of tests/test_gpu_regions.py), against the fp64 oracle
    with the piece path's decisions imposed and against the reference's goldens (the bounds of tests/test_gpu_parity.py);
  * run-to-run identity, the fixed-point run bound on a long single-piece problem, NaN propagation, the model switch and a hipGraph
    capture of a training step."""

import pytest
import torch

import oracle.deform as odeform
from helpers import Golden, assert_zero_grad, decision_tap, params_for, smml, synth
from test_gpu_parity import _calibrated, _compare_param_grads, _load, cpb_probe
from test_oracle_golden import ZERO_GRADS, pathomic_args

pytestmark = pytest.mark.gpu
Fh = smml.functional
NAMES = ("q", "k", "v", "vs", "gq", "w1", "b1", "w2", "b2", "w3", "b3")


def _w1d(kind, gen, hpg=2):
    rn = lambda *s: torch.randn(*s, generator=gen)
    if kind == "torch":        # nn.Linear's default initialisation (what a fresh reference module holds)
        torch.manual_seed(5)
        l1, l2, l3 = torch.nn.Linear(1, 32), torch.nn.Linear(32, 32), torch.nn.Linear(32, hpg)
        return [t.detach().clone() for t in (l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias)]
    if kind == "large":
        return [rn(32, 1) * 4, rn(32) * 3, rn(32, 32) * 2, rn(32) * 2, rn(hpg, 32), rn(hpg)]
    if kind == "kinks2":       # layer-1 kinks spread, layer 2 of mixed sign: many layer-2 zeros
        return [rn(32, 1), rn(32) * 0.6, rn(32, 32), rn(32) * 0.05, rn(hpg, 32) * 0.3, rn(hpg) * 0.1]
    if kind == "w1zero":       # some layer-1 units constant (no kink)
        w = [rn(32, 1) * 0.7, rn(32) * 0.3, rn(32, 32) * 0.25, rn(32) * 0.2, rn(hpg, 32) * 0.3, rn(hpg) * 0.1]
        w[0][::3] = 0.0
        return w
    if kind == "bzero":        # some biases exactly 0: kinks at p = 0
        w = [rn(32, 1) * 0.7, rn(32) * 0.3, rn(32, 32) * 0.25, rn(32) * 0.2, rn(hpg, 32) * 0.3, torch.zeros(hpg)]
        w[1][::2] = 0.0
        w[3][::3] = 0.0
        return w
    if kind == "single":       # no kink at all: one piece covers the line
        return [torch.zeros(32, 1), rn(32).abs() + 0.1, rn(32, 32) * 0.25, rn(32) * 0.2, rn(hpg, 32) * 0.3, rn(hpg) * 0.1]
    return [rn(32, 1) * 0.7, rn(32) * 0.3, rn(32, 32) * 0.25, rn(32) * 0.2, rn(hpg, 32) * 0.3, rn(hpg) * 0.1]


def _restate(w):
    """fp64 restatement of the tables: sorted breakpoints, then per piece its pattern (D1, D2) and (a, c) per output."""
    w1, b1, w2, b2, w3, b3 = (t.double().cpu() for t in w)
    w1 = w1[:, 0]
    nz = w1 != 0
    ks = torch.sort(-b1[nz] / w1[nz]).values
    bps = [ks]
    edges = torch.cat([torch.tensor([-float("inf")], dtype=torch.float64), ks, torch.tensor([float("inf")], dtype=torch.float64)])
    for it in range(len(edges) - 1):
        lo, hi = float(edges[it]), float(edges[it + 1])
        if not lo < hi:
            continue
        x = 0.0 if len(ks) == 0 else (ks[0] - max(1.0, abs(float(ks[0]))) if it == 0 else
                                      (ks[-1] + max(1.0, abs(float(ks[-1]))) if it == len(ks) else 0.5 * (lo + hi)))
        d1 = (w1 * x + b1) > 0
        al = (w2 * (w1 * d1)).sum(1)
        be = (w2 * (b1 * d1)).sum(1) + b2
        z = -be / al
        ok = (al != 0) & (z > lo) & (z < hi)
        bps.append(z[ok])
    bp = torch.sort(torch.cat(bps)).values
    n = len(bp)
    pts = ([0.0] if n == 0 else [float(bp[0]) - max(1.0, abs(float(bp[0])))] + [0.5 * float(bp[i - 1] + bp[i]) for i in range(1, n)] +
           [float(bp[-1]) + max(1.0, abs(float(bp[-1])))])
    p = torch.tensor(pts, dtype=torch.float64)
    x1 = p[:, None] * w1 + b1
    d1 = x1 > 0
    x2 = torch.relu(x1) @ w2.T + b2
    d2 = x2 > 0
    G2 = d2[:, None, :] * w3[None]                                    # [pieces, outputs, 32]
    C1 = (G2 @ w2) * d1[:, None, :]                                   # [pieces, outputs, 32]
    a = (C1 * w1).sum(-1)
    c = (C1 * b1).sum(-1) + (G2 * b2).sum(-1) + b3
    return bp, d1, d2, a, c


def _mlp64(w, p64):
    w1, b1, w2, b2, w3, b3 = (t.double().to(p64.device) for t in w)
    x1 = p64[:, None] * w1[:, 0] + b1
    x2 = torch.relu(x1) @ w2.T + b2
    return x1, x2, torch.relu(x2) @ w3.T + b3


@pytest.mark.parametrize("kind", ["torch", "random", "large", "kinks2", "w1zero", "bzero", "single"])
def test_region1d_tables_match_fp64(cuda, kind):
    gen = torch.Generator().manual_seed(21)
    w = [t.to(cuda).contiguous() for t in _w1d(kind, gen)]
    pmax = 1.6
    tables = Fh.cpb_regions1d_build(*w, pmax)
    torch.cuda.synchronize()
    view = Fh.region1d_tables_view(tables)
    bp, d1, d2, a, c = _restate(w)
    print(f"[{kind}] breakpoints {view['n_bp']} (fp64 restatement {len(bp)})")
    assert view["n_bp"] == len(bp)
    if kind == "single":
        assert view["n_bp"] == 0
    bpd = view["bpd"].cpu()
    assert torch.allclose(bpd, bp, rtol=1e-9, atol=1e-12), "breakpoints differ from the fp64 restatement"
    assert torch.equal(view["bp"].cpu(), bp.float())
    pat = view["pat"].cpu()
    sh = torch.arange(32)
    assert torch.equal(((pat[:, None] >> sh) & 1).bool(), d1), "layer-1 patterns differ"
    assert torch.equal(((pat[:, None] >> (sh + 32)) & 1).bool(), d2), "layer-2 patterns differ"
    coef = view["coef"].cpu().double()
    sa, sc = max(float(a.abs().max()), 1e-30), max(float(c.abs().max()), 1e-30)
    assert float((coef[..., 0] - a).abs().max()) / sa < 2e-6 and float((coef[..., 1] - c).abs().max()) / sc < 2e-6, "(a, c) differ"
    # the kernels' lookup: a forward with queries / sample positions that put >= 1e6 pairs across (and beyond) the grid, plus one key per
    # piece midpoint; its saved piece ids against fp64
    N, J, H = 1024, 1000 + view["n_bp"] + 1, 2
    gq = (torch.rand(N, 1, generator=gen) * 2 - 1).to(cuda)
    vs = torch.rand(1, J, 1, generator=gen) * 8 - 4
    mids = torch.cat([bp[:1] - 0.5, 0.5 * (bp[1:] + bp[:-1]), bp[-1:] + 0.5]) if len(bp) else torch.zeros(1)
    pm = mids.clamp(-3, 3)                                            # offset d with slog(d) = mid for query 0: d = sign(m) (e^|m| - 1)
    vs[0, 1000:, 0] = (gq[0, 0].cpu().double() - torch.sign(pm) * torch.expm1(pm.abs())).float()
    vs = vs.to(cuda)
    z = torch.zeros(1, N, H * 64, device=cuda, requires_grad=True)
    kz = torch.zeros(1, J, H * 64, device=cuda)
    wt = [t.detach().requires_grad_() for t in w]
    with decision_tap() as tap:
        out = Fh.deform_attention(z, kz, kz, vs, gq, *wt, heads=H, groups=1, scale=0.125, cpb_regions=True, cpb_region_pmax=pmax)
        e = tap.entries[-1]
        out.sum().backward()
    torch.cuda.synchronize()
    rid = e["region1d_ids"]
    nst = rid.shape[2] * 32
    ids = (rid[0, 0].permute(0, 2, 1).reshape(nst, J)[:N].long() & 0xFFFF)                      # [N, J]
    d = (gq - vs[0, :, 0][None, :]).double()                                                    # fp32 offsets, as the kernel forms them
    p64 = (torch.sign(d) * torch.log1p(d.abs())).reshape(-1)
    x1, x2, val = _mlp64(w, p64)
    patd = view["pat"][ids.reshape(-1)]
    sh = sh.to(cuda)
    m1, m2 = ((patd[:, None] >> sh) & 1).bool(), ((patd[:, None] >> (sh + 32)) & 1).bool()
    bpc = view["bpd"]
    near = torch.zeros_like(p64, dtype=torch.bool)
    if len(bpc):
        j = torch.searchsorted(bpc, p64).clamp(1, len(bpc)) - 1
        dist = torch.minimum((p64 - bpc[j]).abs(), (p64 - bpc[(j + 1).clamp_max(len(bpc) - 1)]).abs())
        near = dist <= 2e-6 * p64.abs().clamp_min(1.0)
    bad = ((m1 != (x1 > 0)).any(1) | (m2 != (x2 > 0)).any(1)) & ~near
    assert not bool(bad.any()), f"[{kind}] {int(bad.sum())} pairs away from a breakpoint got a piece with other decisions"
    ok = ~near
    coefd = view["coef"].double()[ids.reshape(-1)]                                               # [pairs, outputs, 2]
    got = coefd[..., 0] * p64[:, None] + coefd[..., 1]
    err = float(((got - val).abs() * ok[:, None]).max()) / max(float(val.abs().max()), 1e-30)
    assert err < 2e-6, f"[{kind}] a piece's (a, c) is {err:.2e} off the MLP's value"


def _problem(gen, B, N, J, heads, groups, wkind="random"):
    rn = lambda *s: torch.randn(*s, generator=gen)
    w = _w1d(wkind, gen, heads // groups)
    return dict(q=rn(B, N, heads * 64) * 0.4, k=rn(B, J, heads * 64) * 0.4, v=rn(B, J, heads * 64),
                vs=torch.rand(B * groups, J, 1, generator=gen) * 3 - 1.5, gq=torch.rand(N, 1, generator=gen) * 2 - 1,
                w1=w[0], b1=w[1], w2=w[2], b2=w[3], w3=w[4], b3=w[5])


def _run(t, cuda, wo, regions, heads, groups, p_drop=0.0, seed=3, dout_nan=False):
    dev = {n: x.to(cuda).requires_grad_(n != "gq") for n, x in t.items()}
    kw = {"cpb_regions": True, "cpb_region_pmax": Fh.table_pmax(1.0, 1.5)} if regions else {"cpb_regions": False}
    out = Fh.deform_attention(*(dev[n] for n in NAMES), heads=heads, groups=groups, scale=0.125, dropout_p=p_drop, dropout_seed=seed, **kw)
    w = wo.clone()
    if dout_nan:
        w.view(-1)[7] = float("nan")
    (out * w).sum().backward()
    torch.cuda.synchronize()
    return {n: dev[n].grad.detach().clone() for n in NAMES if n != "gq"} | {"out": out.detach().clone()}


def _torch_ref(t, cuda, wo, heads, groups, p_drop, dt, seed=3):
    """The fused core in plain torch (dtype dt, natural ReLU decisions): gradients of (out * wo).sum()."""
    d = {n: x.to(cuda).to(dt).requires_grad_(n != "gq") for n, x in t.items()}
    B, N, _ = d["q"].shape
    J, H, G, hpg = d["k"].shape[1], heads, groups, heads // groups
    q, k, v = (d[n].view(B, -1, H, 64).permute(0, 2, 1, 3) for n in ("q", "k", "v"))
    off = d["gq"][None, :, None, 0] - d["vs"][:, None, :, 0]                                  # [(B G), N, J]
    p = torch.sign(off) * torch.log1p(off.abs())
    h1 = torch.relu(p[..., None] * d["w1"][:, 0] + d["b1"])
    bias = torch.relu(h1 @ d["w2"].T + d["b2"]) @ d["w3"].T + d["b3"]                        # [(B G), N, J, hpg]
    bias = bias.view(B, G, N, J, hpg).permute(0, 1, 4, 2, 3).reshape(B, H, N, J)
    P = torch.softmax(0.125 * q @ k.transpose(-1, -2) + bias, -1)
    if p_drop:
        P = P * Fh.deform_attention_dropout_mask(B, N, J, H, p_drop, seed, cuda).to(dt) / (1 - p_drop)
    o = (P @ v).permute(0, 2, 1, 3).reshape(B, N, H * 64)
    (o * wo.to(dt)).sum().backward()
    return {n: d[n].grad for n in NAMES if n != "gq"} | {"out": o.detach()}


@pytest.mark.parametrize("heads,groups", [(8, 8), (8, 4)])
@pytest.mark.parametrize("B,N,J,p_drop", [(2, 5, 1, 0.0), (1, 1, 33, 0.0), (2, 129, 33, 0.25), (2, 700, 625, 0.25), (1, 2501, 2501, 0.0),
                                          (1, 129, 2501, 0.25)])
def test_region1d_core_matches_per_pair_mlp(cuda, heads, groups, B, N, J, p_drop):
    """Same inputs through the piece kernels and through the per-pair MLP kernels: out, dq, dk, dv within 2e-5 of their scale of each
    other (test_region_core_matches_per_pair_mlp's bound).  d vs and the parameter gradients are sums over many pairs whose d scores cancel
    (they sum to zero per query): both paths sit at about the same distance from fp64 there (measured, e.g. d vs 4.3e-3 / 5.6e-3 of its
    scale at 2 x 700 x 625), so each of them passes against the per-pair kernels (that test's bounds) OR against plain torch in fp64 (the
    parity policy of tests/test_gpu_parity.py, fp32 torch as the noise reference).  The piece path is run-to-run identical."""
    gen = torch.Generator().manual_seed(300 + N + J + heads // groups)
    t = _problem(gen, B, N, J, heads, groups)
    wo = torch.randn(B, N, heads * 64, generator=gen).to(cuda)
    a = _run(t, cuda, wo, True, heads, groups, p_drop)
    b = _run(t, cuda, wo, False, heads, groups, p_drop)
    for n in ("out", "q", "k", "v"):
        err = float((a[n] - b[n]).abs().max()) / max(float(b[n].abs().max()), 1e-30)
        assert err <= 2e-5, f"{heads}/{groups} {B}x{N}x{J}: {n} differs by {err:.2e} of its scale between the piece and the per-pair kernels"
    r32 = _torch_ref(t, cuda, wo, heads, groups, p_drop, torch.float32)
    r64 = _torch_ref(t, cuda, wo, heads, groups, p_drop, torch.float64)
    for n in ("vs", "w1", "b1", "w2", "b2", "w3"):      # (d b3 = sum of all d scores: zero in exact arithmetic)
        # either yardstick: the per-pair kernels at test_region_core_matches_per_pair_mlp's bounds, or fp64 at the parity policy.  Where
        # one of them fails the other path is the less exact one: the per-pair MLP's own rounding (e.g. d W2 2.3e-3 of its scale from fp64
        # at 2 501 x 2 501, the piece path 6e-4), or a pair within rounding of a breakpoint decided the other way than fp64 decides it
        # (its slope jumps there: visible in d vs at J > 768, as in the 2-D test)
        err = float((a[n] - b[n]).abs().max()) / max(float(b[n].abs().max()), 1e-30)
        tol = (2e-2 if n == "vs" else 2e-3) if J > 768 else 5e-4
        if err <= tol:
            continue
        try:
            _calibrated(f"{heads}/{groups} {B}x{N}x{J} d{n}", a[n], r32[n], r64[n])
        except AssertionError as e:
            raise AssertionError(f"{heads}/{groups} {B}x{N}x{J}: d{n} differs by {err:.2e} > {tol:.0e} of its scale from the per-pair "
                                 f"kernels, and from fp64: {e}") from None
    a2 = _run(t, cuda, wo, True, heads, groups, p_drop)
    for n in a:
        assert torch.equal(a[n], a2[n]), f"{n}: the piece path is not run-to-run identical"


def test_region1d_long_single_piece_run_bound_and_nan(cuda):
    """One piece covers every pair, so a key's run of equal piece ids is as long as its queries: the runs are flushed at every 32-query
    tile, and the moments of N = 10 001 queries x 2 500 keys x B G = 8 stay exact (against the per-pair kernels, test 2's bounds).  A NaN
    d score makes the six parameter gradients NaN."""
    gen = torch.Generator().manual_seed(77)
    B, N, J, H, G = 2, 10001, 2500, 8, 4
    t = _problem(gen, B, N, J, H, G, "single")
    wo = torch.randn(B, N, H * 64, generator=gen).to(cuda)
    a = _run(t, cuda, wo, True, H, G)
    b = _run(t, cuda, wo, False, H, G)
    # with w1 = 0 layer 1 is constant: every parameter gradient but d w1 is linear in M0 = sum of the d scores, zero in exact arithmetic
    # (the softmax's rows sum to one) - rounding in both paths, as d b3 everywhere.  d w1 = C1 . M1 and d vs carry the moments.
    for n in ("w1", "vs"):
        err = float((a[n] - b[n]).abs().max()) / max(float(b[n].abs().max()), 1e-30)
        print(f"single piece: {n} {err:.2e}")
        assert err <= (2e-2 if n == "vs" else 2e-3), f"{n} differs by {err:.2e} of its scale on the single-piece problem"
    gen = torch.Generator().manual_seed(78)
    t = _problem(gen, 1, 70, 40, 8, 4)
    c = _run(t, cuda, torch.randn(1, 70, 512, generator=gen).to(cuda), True, 8, 4, dout_nan=True)
    for n in ("w1", "b1", "w2", "b2", "w3", "b3"):
        assert bool(torch.isnan(c[n]).all()), f"d{n} is not NaN after a NaN d score"
    assert bool(torch.isnan(c["vs"]).any()), "d vs shows no NaN after a NaN d score"


class _Decisions1D:
    """helpers.Decisions with the ReLU decisions of the piece path (functional.DECISION_TAP entry 'region1d_ids'): the pattern of each
    pair's piece; the heads of a group share the piece, the first is taken."""

    def __init__(self, dec, entry):
        self.cells, self.N = dec.cells, dec.N
        B, H, G, J = entry["B"], entry["heads"], entry["groups"], entry["J"]
        rid = entry["region1d_ids"]
        nst = rid.shape[2] * 32
        self.rid = rid.view(B, H, nst // 32, J, 32)[:, ::H // G].permute(0, 1, 3, 2, 4).reshape(B * G, J, nst)
        self.pat = Fh.region1d_tables_view(entry["region1d_tables"])["pat"].clone()

    def relu_masks(self, i0, i1, device="cpu"):
        ids = (self.rid[:, :, i0:i1].long() & 0xFFFF).transpose(1, 2)
        words = self.pat[ids]
        sh = torch.arange(32, device=words.device)
        return ((words[..., None] >> sh) & 1).bool().to(device), ((words[..., None] >> (sh + 32)) & 1).bool().to(device)


@pytest.mark.parametrize("B,n", [(2, 5), (1, 64), (3, 129), (2, 300)])
def test_region1d_vs_oracle_with_decisions_imposed(cuda, B, n):
    """test_deform1d_vs_oracle_lengths through DeformCrossAttention1D(cpb_regions=True), with the piece path's decisions imposed."""
    from oracle.deform import deform_cross_attention_1d
    C = 128
    tag = f"d1d:{B}:{n}"
    mod = smml.DeformCrossAttention1D(dim=C, downsample_factor=4, offset_scale=2, offset_kernel_size=6, cpb_regions=True)
    params = params_for(mod, 9, tag)
    mod = _load(mod, params, cuda)
    x1 = synth.normal((B, C, n), 9, tag + ":x1"); x2 = synth.normal((B, C, n), 9, tag + ":x2")
    wo = synth.normal((B, C, n), 9, tag + ":wo")
    ad, bd = x1.to(cuda).requires_grad_(), x2.to(cuda).requires_grad_()
    with decision_tap() as tap:
        o, vg = mod(ad, bd, return_vgrid=True)
        entries = list(tap.entries)
    assert entries[1].get("region1d_ids") is not None, "the module did not take the piece path"
    w_vg = synth.normal(tuple(vg.shape), 9, tag + ":wvg")
    ((o * wo.to(cuda)).sum() + (vg * w_vg.to(cuda)).sum()).backward()
    dec = [_Decisions1D(d, entries[1]) for d in tap.decisions()]
    run = {}
    with cpb_probe() as probe:
        for dt in (torch.float32, torch.float64):
            pref = {k: v.clone().to(dt).requires_grad_() for k, v in params.items()}
            a, b = x1.clone().to(dt).requires_grad_(), x2.clone().to(dt).requires_grad_()
            odeform.DECISIONS = list(dec)
            o_ref, vg_ref = deform_cross_attention_1d(a, b, pref, downsample_factor=4, offset_scale=2, offset_kernel_size=6)
            ((o_ref * wo.to(dt)).sum() + (vg_ref * w_vg.to(dt)).sum()).backward()
            run[dt] = (o_ref, vg_ref, a.grad, b.grad, pref)
    r32, r64 = run[torch.float32], run[torch.float64]
    for name, got, i in (("out", o, 0), ("vgrid", vg, 1), ("dx1", ad.grad, 2), ("dx2", bd.grad, 3)):
        _calibrated(name, got, r32[i], r64[i])
    _compare_param_grads(mod, r32[4], r64[4], probe=probe)


@pytest.mark.parametrize("tag,B,n", [("deform1d_n37", 2, 37), ("deform1d_n40", 2, 40), ("deform1d_n2501", 1, 2501)])
def test_region1d_golden(cuda, tag, B, n):
    """test_deform1d_golden through DeformCrossAttention1D(cpb_regions=True): the reference's own outputs, nothing imposed."""
    g = Golden(tag)
    C = 128
    mod = smml.DeformCrossAttention1D(dim=C, downsample_factor=4, offset_scale=2, offset_kernel_size=6, cpb_regions=True)
    mod = _load(mod, params_for(mod, 42, tag), cuda)
    x1 = synth.normal((B, C, n), 42, tag + ":x1").to(cuda).requires_grad_()
    x2 = synth.normal((B, C, n), 42, tag + ":x2").to(cuda).requires_grad_()
    w_out = synth.normal((B, C, n), 42, tag + ":wout").to(cuda)
    out, vgrid = mod(x1, x2, return_vgrid=True)
    w_vg = synth.normal(tuple(vgrid.shape), 42, tag + ":wvg").to(cuda)
    ((out * w_out).sum() + (vgrid * w_vg).sum()).backward()
    g.check("out", out); g.check("vgrid", vgrid); g.check("dx1", x1.grad); g.check("dx2", x2.grad)
    for k, p in mod.named_parameters():
        if k.endswith(ZERO_GRADS):
            assert_zero_grad(f"{g.name}:d{k}", p.grad, g.scalar("natural:" + k))
        else:
            g.check("grad:" + k, p.grad, what="d" + k)


def _pathomic(cuda, key, dropout_rate=0.1):
    net = smml.DeformPathomicNet(pathomic_args(attn_dim=1, return_vgrid=False, deform1d_cpb_regions=key, dropout_rate=dropout_rate))
    return _load(net, params_for(net, 42, "pathomic"), cuda)


def _step(net, x_path, x_t, x_i, label):
    feats, vt, vi, lg, _, _, _ = net(x_path=x_path, x_omic=None, x_omic_tumor=x_t, x_omic_immune=x_i)
    return torch.nn.functional.cross_entropy(lg[2], label) + feats.pow(2).mean()


def _inputs(cuda, B=2, n=2500):
    return (synth.bag(B, n, 1024, 42, "pathomic:bag").to(cuda), synth.normal((B, 59), 42, "pathomic:tumor").to(cuda),
            synth.normal((B, 361), 42, "pathomic:immune").to(cuda), torch.tensor([1, 3], device=cuda))


def test_region1d_pathomic_step_key_true_vs_false(cuda):
    """One training step of DeformPathomicNet with attn_dim = 1 at N = 2 500, deform1d_cpb_regions True vs False: the loss within 2e-5 of
    its scale, every parameter gradient within 5e-4 of its scale."""
    x = _inputs(cuda)
    res = {}
    for key in (False, True):
        net = _pathomic(cuda, key)
        torch.manual_seed(0)
        loss = _step(net, *x)
        loss.backward()
        torch.cuda.synchronize()
        res[key] = (float(loss.detach()), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None})
    la, lb = res[True][0], res[False][0]
    assert abs(la - lb) <= 2e-5 * max(abs(lb), 1e-30), f"loss {la} vs {lb}"
    assert res[True][1].keys() == res[False][1].keys()
    for k, gb in res[False][1].items():
        ga = res[True][1][k]
        scale = float(gb.abs().max())
        if scale < 1e-12 or k.endswith("rel_pos_bias.mlp.2.bias"):     # d b3: the sum of all d scores, zero in exact arithmetic
            continue
        err = float((ga - gb).abs().max()) / scale
        assert err <= 5e-4, f"d{k} differs by {err:.2e} of its scale with the key True"


def test_region1d_pathomic_step_in_a_graph(cuda):
    """A whole training step with the key True captured in a hipGraph: a replay gives the eager step's loss and gradients."""
    x = _inputs(cuda)
    net = _pathomic(cuda, True, dropout_rate=0.0)
    params = [p for p in net.parameters()]

    def step():
        for p in params:
            p.grad = None
        loss = _step(net, *x)
        loss.backward()
        return loss

    loss_e = step().detach().clone()
    torch.cuda.synchronize()
    grads_e = [None if p.grad is None else p.grad.detach().clone() for p in params]
    s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                                        # warm-up on the capture stream
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            loss_g = step()
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss_g.detach(), loss_e), f"graph loss {float(loss_g)} vs eager {float(loss_e)}"
    for p, ge in zip(params, grads_e):
        if ge is None:
            continue
        scale = max(float(ge.abs().max()), 1e-30)
        err = float((p.grad - ge).abs().max()) / scale
        assert err <= 2e-5, f"a gradient of the replay differs from eager by {err:.2e} of its scale"
