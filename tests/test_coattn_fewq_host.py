"""CPU: the host side of the few-query co-attention (functional.coattn_path / coattn_why / few_query_attention's shape errors,
MultiheadAttention.fused_few_query, CMTA's extension key `coattn_fused`, the four C-ABI entries of csrc/fewq_attn.hip) - no device - and
the algebra of the folded form against oracle.coattn.coattention in fp64."""
import argparse
import inspect

import pytest
import torch

from helpers import header_arity, smml
from oracle.coattn import coattention

Fh = smml.functional
FEWQ_SYMBOLS = {"smml_fewq_attn_fwd_workspace_bytes": 5, "smml_fewq_attn_fwd_f32": 21, "smml_fewq_attn_bwd_workspace_bytes": 5,
                "smml_fewq_attn_bwd_f32": 30}
BASE = dict(L=4, heads=1, Ek=256, Ev=256)


@pytest.mark.parametrize("L", [1, 4, 8])
def test_few_queries_with_one_head_take_the_kernels(L):
    assert Fh.coattn_path(**dict(BASE, L=L)) == "fewq"
    assert Fh.coattn_why(**dict(BASE, L=L)) is None
    assert Fh.coattn_path(L=L, heads=1, Ek=64, Ev=512) == "fewq"


@pytest.mark.parametrize("over, word", [(dict(L=9), "queries"), (dict(heads=2), "heads"), (dict(attn_mask=True), "attn_mask"),
                                        (dict(add_bias_kv=True), "add_bias_kv"), (dict(add_zero_attn=True), "add_zero_attn"),
                                        (dict(dropout_active=True), "dropout"), (dict(Ek=96), "widths"), (dict(Ev=96), "widths"),
                                        (dict(Ek=576), "widths"), (dict(fused=False), "off")])
def test_everything_else_stays_composed_with_a_reason(over, word):
    kw = dict(BASE, **over)
    assert Fh.coattn_path(**kw) == "composed"
    assert word in Fh.coattn_why(**kw)


def test_c_abi_declares_the_four_entries():
    arity = header_arity()
    for name, n in FEWQ_SYMBOLS.items():
        assert name in smml.SIGNATURES, name
        assert len(smml.SIGNATURES[name][1]) == arity[name] == n, name


def test_flag_is_an_attribute_not_state():
    plain, flagged = smml.MultiheadAttention(256, 1), smml.MultiheadAttention(256, 1)
    assert plain.fused_few_query is False and plain.fewq_splits is None
    flagged.fused_few_query, flagged.fewq_splits = True, 7
    assert list(flagged.state_dict()) == list(plain.state_dict()) == ["in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias"]
    flagged.load_state_dict(plain.state_dict(), strict=True)
    assert list(inspect.signature(smml.MultiheadAttention.__init__).parameters) == [
        "self", "embed_dim", "num_heads", "dropout", "bias", "add_bias_kv", "add_zero_attn", "kdim", "vdim"]


def test_cmta_reads_the_extension_key():
    off = smml.CMTA(argparse.Namespace(label_dim=4))
    false = smml.CMTA(argparse.Namespace(label_dim=4, coattn_fused=False))
    on = smml.CMTA(argparse.Namespace(label_dim=4, coattn_fused=True))
    assert off.G_in_P_Att.fused_few_query is False and false.G_in_P_Att.fused_few_query is False
    assert on.G_in_P_Att.fused_few_query is True
    assert on.P_in_G_Att.fused_few_query is False          # many queries over 4 keys: the dual problem stays composed
    assert list(on.state_dict()) == list(off.state_dict())


def test_unsupported_sizes_raise_before_any_launch():
    x = torch.zeros(2, 5, 256)
    with pytest.raises(ValueError, match="at most 8 queries"):
        Fh.few_query_attention(torch.zeros(2, 9, 256), torch.zeros(2, 9), x)
    with pytest.raises(ValueError, match="multiples of 64"):
        Fh.few_query_attention(torch.zeros(2, 4, 96), torch.zeros(2, 4), torch.zeros(2, 5, 96))
    with pytest.raises(ValueError, match="multiples of 64"):
        Fh.few_query_attention(torch.zeros(2, 4, 256), torch.zeros(2, 4), x, torch.zeros(2, 5, 576))
    with pytest.raises(ValueError, match="one problem"):
        Fh.few_query_attention(torch.zeros(2, 4, 256), torch.zeros(2, 3), x)
    with pytest.raises(ValueError, match="key_padding_mask"):
        Fh.few_query_attention(torch.zeros(2, 4, 256), torch.zeros(2, 4), x, key_padding_mask=torch.zeros(2, 6, dtype=torch.bool))


def test_workspace_sizes():
    lib = smml.lib()
    assert lib.smml_fewq_attn_fwd_workspace_bytes(3, 4, 300, 256, 7) == 3 * 7 * 4 * (256 + 4) * 4
    assert lib.smml_fewq_attn_bwd_workspace_bytes(3, 4, 300, 256, 7) == 3 * 7 * 4 * (256 + 4) * 4
    assert lib.smml_fewq_attn_fwd_workspace_bytes(2, 6, 300, 128, 300) == 2 * 300 * 6 * (128 + 4) * 4
    assert lib.smml_fewq_attn_fwd_workspace_bytes(8, 4, 10000, 256, 0) == 8 * 127 * 4 * (256 + 4) * 4     # 128 wanted, 79 rows each
    assert lib.smml_fewq_attn_fwd_workspace_bytes(2, 4, 11, 256, 0) == 2 * 1 * 4 * (256 + 4) * 4          # never under 64 rows
    assert lib.smml_fewq_attn_fwd_workspace_bytes(0, 4, 11, 256, 0) == 0


def folded(q, kv, p, kpm=None):
    """The folded form in plain torch, as MultiheadAttention._forward_few_query composes it around the core."""
    E = q.shape[-1]
    w, b = p["in_proj_weight"], p["in_proj_bias"]
    qh = (q.transpose(0, 1) @ w[:E].t() + b[:E]) * E ** -0.5
    u, c = qh @ w[E:2 * E], qh @ b[E:2 * E]
    x = kv.transpose(0, 1)
    raw = u @ x.transpose(1, 2) + c[..., None]
    if kpm is not None:
        raw = raw.masked_fill(kpm[:, None, :], float("-inf"))
    z = torch.softmax(raw, -1) @ x
    o = z @ w[2 * E:].t() + b[2 * E:]
    return (o @ p["out_proj.weight"].t() + p["out_proj.bias"]).transpose(0, 1), raw[:, None]


def test_folded_form_is_the_oracle_in_fp64():
    """The written record of the algebra the kernels rely on (`folded` above against the oracle, outputs and every gradient, with a mask).
    It runs no project code and holds on any revision; the GPU file tests the kernels against the same oracle."""
    L, S, B, E = 4, 50, 2, 64
    g = torch.Generator().manual_seed(5)
    p = {"in_proj_weight": torch.randn(3 * E, E, generator=g, dtype=torch.float64) / 8, "in_proj_bias": torch.randn(3 * E, generator=g, dtype=torch.float64),
         "out_proj.weight": torch.randn(E, E, generator=g, dtype=torch.float64) / 8, "out_proj.bias": torch.randn(E, generator=g, dtype=torch.float64)}
    q, kv = torch.randn(L, B, E, generator=g, dtype=torch.float64), torch.randn(S, B, E, generator=g, dtype=torch.float64)
    wo, wr = torch.randn(L, B, E, generator=g, dtype=torch.float64), torch.randn(B, 1, L, S, generator=g, dtype=torch.float64)
    kpm = torch.zeros(B, S, dtype=torch.bool); kpm[0, 3:9] = True; kpm[1, -1] = True
    res = []
    for fn in (lambda a, b_, c_: coattention(a, b_, b_, c_, key_padding_mask=kpm), lambda a, b_, c_: folded(a, b_, c_, kpm)):
        leaves = [t.clone().requires_grad_() for t in (q, kv, *p.values())]
        out, raw = fn(leaves[0], leaves[1], dict(zip(p, leaves[2:])))
        fin = torch.isfinite(raw)
        ((out * wo).sum() + (torch.where(fin, raw, torch.zeros_like(raw)) * wr).sum() * 1e-2).backward()
        res.append([out.detach(), torch.where(fin, raw, torch.zeros_like(raw)).detach()] + [t.grad for t in leaves])
        assert int((~fin).sum()) == L * 7
    for a, b_ in zip(*res):
        assert float((a - b_).abs().max()) <= 1e-12 * max(1.0, float(b_.abs().max()))


def test_values_are_the_keys_only_where_the_gradient_may_be_shared():
    """The one-read / one-row form is for the same tensor, two views of one base, or aliases without gradients; a detached alias on one
    side keeps the distinct form (the side that requires a gradient gets its own part alone)."""
    same = Fh._same_rows
    kv = torch.randn(5, 2, 64, requires_grad=True)
    x = kv.transpose(0, 1)
    assert same(x, None) and same(x, x) and same(x, kv.transpose(0, 1))
    assert same(kv.detach(), kv.detach())
    assert not same(x, kv.detach().transpose(0, 1)) and not same(kv.detach().transpose(0, 1), x)
    assert not same(kv, kv.detach()) and not same(kv.detach(), kv)
    assert not same(x, torch.randn(2, 5, 64))
    y = Fh._value_rows(kv.detach(), kv.detach())             # aliased values in the distinct form are copied: the C side reads y == x as one row
    assert y.data_ptr() != kv.data_ptr() and torch.equal(y, kv)
    other = torch.randn(5, 2, 64)
    assert Fh._value_rows(kv.detach(), other) is other
