"""GPU: the streaming kernels of the grouped 1x1 convolutions (csrc/grouped_pointwise.hip; to_q / to_k / to_v, 16 -> 64 channels per group).

  * forward and dX carry the BITS of the batched-GEMM route they replace (functional._gemm with _GroupedPointwise's arguments, one batch
    item per group): torch.equal, and within 1e-5 of the tensor's scale of an fp64 product (the bound of the GEMM cases of test_gpu_parity);
  * dW is within that bound of fp64 and the same bits on every call, with the deterministic switch on or off (one form: per-workgroup
    partials added in a fixed order);
  * functional.grouped_pointwise through autograd on a shape the kernels take and on one they must leave to the batched route.
Row counts: one row, both sides of the 32-row tile and of 128, several tiles (300, 700).  dW cuts the rows into workgroups of 16 rows at
these sizes (700 rows: 44 partials, so the second kernel and its eight segments run), and every count that is no multiple of 16 ends in
a partly filled step.  One longer case (16 500 rows at G = 8) makes a forward / dX workgroup take a second tile and a dW workgroup a second
and third step: the loops whose next operands are requested ahead of the MFMAs."""
import pytest
import torch

from helpers import assert_close, smml

pytestmark = pytest.mark.gpu
Fh = smml.functional
capi = smml._capi

ROWS = (1, 31, 32, 33, 127, 129, 300, 700)
LONG = 16500      # G = 8 only: more 32-row tiles (516) than row-striding workgroups (512) and three 16-row steps per dW workgroup
GROUPS = (1, 2, 8)
CIN_G, COUT_G = 16, 64
TOL = 1e-5        # of the tensor's scale: the bound of the GEMM cases of tests/test_gpu_parity.py


def _case(rows, G, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, G * CIN_G, generator=gen)
    w = torch.randn(G * COUT_G, CIN_G, generator=gen) * 0.25
    dy = torch.randn(rows, G * COUT_G, generator=gen)
    return x, w, dy


def _ref64(x, w, dy, G):
    """fp64: y [rows, G 64], dx [rows, G 16], dw [G 64, 16]"""
    x3, w3, dy3 = x.double().view(-1, G, CIN_G), w.double().view(G, COUT_G, CIN_G), dy.double().view(-1, G, COUT_G)
    y = torch.einsum("mgi,goi->mgo", x3, w3).reshape(-1, G * COUT_G)
    dx = torch.einsum("mgo,goi->mgi", dy3, w3).reshape(-1, G * CIN_G)
    dw = torch.einsum("mgo,mgi->goi", dy3, x3).reshape(G * COUT_G, CIN_G)
    return y, dx, dw


def _batched_route(x, w, dy, G):
    """forward and dX as _GroupedPointwise issues them on the batched-GEMM route"""
    rows, Cin, Cout = x.shape[0], G * CIN_G, G * COUT_G
    y, dx = torch.empty(rows, Cout, device=x.device), torch.empty(rows, Cin, device=x.device)
    Fh._gemm(x, w, y, M=rows, N=COUT_G, K=CIN_G, sam=Cin, sak=1, sbk=1, sbn=CIN_G, ldc=Cout, nb1=G,
             sa1=CIN_G, sb1=COUT_G * CIN_G, sc1=COUT_G)
    Fh._gemm(dy, w, dx, M=rows, N=CIN_G, K=COUT_G, sam=Cout, sak=1, sbk=CIN_G, sbn=1, ldc=Cin, nb1=G,
             sa1=COUT_G, sb1=COUT_G * CIN_G, sc1=CIN_G)
    return y, dx


def _streaming_fwd_dx(x, w, dy, G):
    L = capi.lib()
    rows = x.shape[0]
    y, dx = torch.empty(rows, G * COUT_G, device=x.device), torch.empty(rows, G * CIN_G, device=x.device)
    capi.check(L.smml_grouped_pointwise_fwd_f32(capi.fptr(x), capi.fptr(w), capi.fptr(y), rows, G, CIN_G, COUT_G, capi.stream()), "fwd")
    capi.check(L.smml_grouped_pointwise_dx_f32(capi.fptr(dy), capi.fptr(w), capi.fptr(dx), rows, G, CIN_G, COUT_G, capi.stream()), "dx")
    return y, dx


def _streaming_dw(x, dy, G):
    L = capi.lib()
    rows = x.shape[0]
    dw = torch.full((G * COUT_G, CIN_G), float("nan"), device=x.device)       # overwritten, never accumulated into
    wsb = L.smml_grouped_pointwise_dw_workspace_bytes(rows, G, CIN_G, COUT_G)
    assert wsb > 0
    ws = torch.full(((wsb + 3) // 4,), float("nan"), device=x.device)
    capi.check(L.smml_grouped_pointwise_dw_f32(capi.fptr(dy), capi.fptr(x), capi.fptr(dw), rows, G, CIN_G, COUT_G, capi.fptr(ws), wsb,
                                               capi.stream()), "dw")
    return dw


@pytest.mark.parametrize("G", GROUPS)
def test_grouped_forward_and_dx_carry_the_bits_of_the_batched_route(cuda, G):
    assert capi.lib().smml_grouped_pointwise_applies(G, CIN_G, COUT_G) == 1
    for rows in ROWS + ((LONG,) if G == 8 else ()):
        x, w, dy = _case(rows, G, 1000 * G + rows)
        y64, dx64, _ = _ref64(x, w, dy, G)
        xd, wd, dyd = x.to(cuda), w.to(cuda), dy.to(cuda)
        y_b, dx_b = _batched_route(xd, wd, dyd, G)
        y_s, dx_s = _streaming_fwd_dx(xd, wd, dyd, G)
        print(f"rows {rows} G {G}: y differs in {int((y_s != y_b).sum())} of {y_s.numel()}, dx in {int((dx_s != dx_b).sum())} of {dx_s.numel()}")
        assert torch.equal(y_s, y_b), f"forward, rows {rows}, G {G}: not the bits of the batched route"
        assert torch.equal(dx_s, dx_b), f"dX, rows {rows}, G {G}: not the bits of the batched route"
        assert_close(f"grouped fwd rows {rows} G {G} vs fp64", y_s, y64, TOL)
        assert_close(f"grouped dx rows {rows} G {G} vs fp64", dx_s, dx64, TOL)


@pytest.mark.parametrize("G", GROUPS)
def test_grouped_dw_is_exact_and_the_same_bits_in_both_modes(cuda, G):
    for rows in ROWS + ((LONG,) if G == 8 else ()):
        x, w, dy = _case(rows, G, 2000 * G + rows)
        _, _, dw64 = _ref64(x, w, dy, G)
        xd, wd, dyd = x.to(cuda), w.to(cuda), dy.to(cuda)
        got = []
        for det in (False, True, False, True):
            with smml.deterministic(det):
                got.append(_streaming_dw(xd, dyd, G))
                xl, wl = xd.clone().requires_grad_(), wd.clone().requires_grad_()
                yl = Fh.grouped_pointwise(xl, wl, G)
            yl.backward(dyd)
            got.append(wl.grad)
        assert_close(f"grouped dw rows {rows} G {G} vs fp64", got[0], dw64, TOL)
        for i, g in enumerate(got[1:]):
            assert torch.equal(g, got[0]), f"dW, rows {rows}, G {G}: call {i + 1} differs from the first call"


@pytest.mark.parametrize("cin_g,streaming", [(16, True), (12, False)])
def test_grouped_pointwise_autograd(cuda, cin_g, streaming):
    """rows 300, G = 8: 16 input channels per group take the streaming kernels, 12 stay on the batched route; both against an fp64 einsum"""
    G, rows = 8, 300
    assert bool(capi.lib().smml_grouped_pointwise_applies(G, cin_g, COUT_G)) == streaming
    gen = torch.Generator().manual_seed(77 + cin_g)
    x = torch.randn(2, rows // 2, G * cin_g, generator=gen)
    w = torch.randn(G * COUT_G, cin_g, 1, generator=gen) * 0.25              # a Conv1d weight [Cout, Cin / groups, 1]
    dy = torch.randn(2, rows // 2, G * COUT_G, generator=gen)
    x3, w3, dy3 = x.double().view(rows, G, cin_g), w.double().view(G, COUT_G, cin_g), dy.double().view(rows, G, COUT_G)
    y64 = torch.einsum("mgi,goi->mgo", x3, w3).reshape(2, rows // 2, -1)
    dx64 = torch.einsum("mgo,goi->mgi", dy3, w3).reshape(2, rows // 2, -1)
    dw64 = torch.einsum("mgo,mgi->goi", dy3, x3).reshape(G * COUT_G, cin_g, 1)
    xl, wl = x.to(cuda).requires_grad_(), w.to(cuda).requires_grad_()
    y = Fh.grouped_pointwise(xl, wl, G)
    y.backward(dy.to(cuda))
    assert y.shape == y64.shape and xl.grad.shape == x.shape and wl.grad.shape == w.shape
    assert_close(f"grouped_pointwise y cin_g {cin_g}", y, y64, TOL)
    assert_close(f"grouped_pointwise dx cin_g {cin_g}", xl.grad, dx64, TOL)
    assert_close(f"grouped_pointwise dw cin_g {cin_g}", wl.grad, dw64, TOL)
