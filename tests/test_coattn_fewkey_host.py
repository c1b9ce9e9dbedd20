"""CPU: the host side of the few-key co-attention (functional.coattn_few_key_why / few_key_attention's shape errors,
MultiheadAttention.fused_few_key, CMTA's extension key `coattn_fused_few_key`, the four C-ABI entries of csrc/fewk_attn.hip) - no device -
and the algebra of the folded form against oracle.coattn.coattention in fp64."""
import argparse
import inspect

import pytest
import torch

from helpers import header_arity, smml
from oracle.coattn import coattention

Fh, capi = smml.functional, smml._capi
FEWK_SYMBOLS = {"smml_fewk_attn_fwd_workspace_bytes": 5, "smml_fewk_attn_fwd_f32": 18, "smml_fewk_attn_bwd_workspace_bytes": 6,
                "smml_fewk_attn_bwd_f32": 25}
CMTA_CALL = dict(S=4, heads=1, Eq=256, attn_mask=False, add_bias_kv=False, add_zero_attn=False, dropout_active=False, fused=True)


def test_c_abi_declares_the_four_entries():
    arity = header_arity()
    for name, n in FEWK_SYMBOLS.items():
        assert name in smml.SIGNATURES, name
        assert len(smml.SIGNATURES[name][1]) == arity[name] == n, name
    assert smml._capi.ABI_VERSION == 2


def test_launch_namespaces_cover_the_header_and_have_no_dead_key():
    names = lambda proto: {n for n, _, _ in capi.PARAMS[proto]}          # noqa: E731
    assert Fh.FEWK_FWD_KEYS == names("smml_fewk_attn_fwd_f32")
    assert Fh.FEWK_BWD_KEYS == names("smml_fewk_attn_bwd_f32")


@pytest.mark.parametrize("S", [1, 3, 4, 8])
def test_few_keys_with_one_head_take_the_kernels(S):
    assert Fh.coattn_few_key_why(**dict(CMTA_CALL, S=S)) is None
    assert Fh.coattn_few_key_why(S=S, heads=1, Eq=64) is None and Fh.coattn_few_key_why(S=S, heads=1, Eq=512) is None


@pytest.mark.parametrize("over, word", [(dict(S=9), "keys"), (dict(S=0), "keys"), (dict(heads=2), "heads"), (dict(attn_mask=True), "attn_mask"),
                                        (dict(add_bias_kv=True), "add_bias_kv"), (dict(add_zero_attn=True), "add_zero_attn"),
                                        (dict(dropout_active=True), "dropout"), (dict(Eq=96), "width"), (dict(Eq=576), "width"),
                                        (dict(fused=False), "off")])
def test_everything_else_stays_composed_with_a_reason(over, word):
    why = Fh.coattn_few_key_why(**dict(CMTA_CALL, **over))
    assert why is not None and word in why


@pytest.mark.parametrize("L", [1, 4, 8])
def test_few_query_routing_is_unchanged(L):
    base = dict(L=L, heads=1, Ek=256, Ev=256)
    assert Fh.coattn_path(**base) == "fewq" and Fh.coattn_why(**base) is None
    assert Fh.coattn_path(L=L, heads=1, Ek=64, Ev=512) == "fewq"
    for over, word in ((dict(L=9), "queries"), (dict(heads=2), "heads"), (dict(attn_mask=True), "attn_mask"), (dict(Ek=96), "widths"),
                       (dict(dropout_active=True), "dropout"), (dict(fused=False), "off")):
        assert Fh.coattn_path(**dict(base, **over)) == "composed" and word in Fh.coattn_why(**dict(base, **over))
    assert list(inspect.signature(Fh.coattn_why).parameters) == ["L", "heads", "Ek", "Ev", "attn_mask", "add_bias_kv", "add_zero_attn",
                                                                 "dropout_active", "fused"]


def test_unsupported_sizes_raise_before_any_launch():
    """CPU and meta tensors: nothing here could be launched, and the library is not asked."""
    def call(B=2, L=5, S=4, Eq=256, Eo=256, Bu=None, device="cpu", **kw):
        z = lambda *s: torch.zeros(*s, device=device)          # noqa: E731
        return Fh.few_key_attention(z(B, L, Eq), z(Bu or B, S, Eq), z(Bu or B, S), z(Bu or B, S, Eo), **kw)

    for device in ("cpu", "meta"):
        with pytest.raises(ValueError, match="between 1 and 8 keys"):
            call(S=0, device=device)
        with pytest.raises(ValueError, match="between 1 and 8 keys"):
            call(S=9, device=device)
        with pytest.raises(ValueError, match="multiples of 64"):
            call(Eq=96, device=device)
        with pytest.raises(ValueError, match="multiples of 64"):
            call(Eo=576, device=device)
        with pytest.raises(ValueError, match="one problem"):
            call(Bu=3, device=device)
    with pytest.raises(ValueError, match="key_padding_mask"):
        call(key_padding_mask=torch.zeros(2, 5, dtype=torch.bool))
    with pytest.raises(ValueError, match="empty bag"):
        call(L=0)


def test_flag_is_an_attribute_not_state():
    plain, flagged = smml.MultiheadAttention(256, 1), smml.MultiheadAttention(256, 1)
    assert plain.fused_few_key is False and plain.fewk_splits is None
    assert plain.fused_few_query is False and plain.fewq_splits is None
    flagged.fused_few_key, flagged.fewk_splits = True, 7
    assert list(flagged.state_dict()) == list(plain.state_dict()) == ["in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias"]
    flagged.load_state_dict(plain.state_dict(), strict=True)
    assert list(inspect.signature(smml.MultiheadAttention.__init__).parameters) == [
        "self", "embed_dim", "num_heads", "dropout", "bias", "add_bias_kv", "add_zero_attn", "kdim", "vdim"]


def test_cmta_reads_the_extension_key():
    ns = lambda **kw: argparse.Namespace(label_dim=4, **kw)          # noqa: E731
    off, false, on = smml.CMTA(ns()), smml.CMTA(ns(coattn_fused_few_key=False)), smml.CMTA(ns(coattn_fused_few_key=True))
    both, fewq = smml.CMTA(ns(coattn_fused=True, coattn_fused_few_key=True)), smml.CMTA(ns(coattn_fused=True))
    assert off.P_in_G_Att.fused_few_key is False and false.P_in_G_Att.fused_few_key is False
    assert on.P_in_G_Att.fused_few_key is True and on.G_in_P_Att.fused_few_key is False and on.G_in_P_Att.fused_few_query is False
    assert both.P_in_G_Att.fused_few_key is True and both.G_in_P_Att.fused_few_query is True
    assert fewq.P_in_G_Att.fused_few_key is False and fewq.G_in_P_Att.fused_few_query is True       # coattn_fused: the few-query side only
    assert list(on.state_dict()) == list(off.state_dict())
    mod = on.P_in_G_Att
    assert Fh.coattn_few_key_why(S=len(on.omic_sizes), heads=mod.num_heads, Eq=mod.embed_dim, attn_mask=False, add_bias_kv=mod.bias_k is not None,
                                 add_zero_attn=mod.add_zero_attn, dropout_active=mod.dropout > 0, fused=mod.fused_few_key) is None


def test_workspace_sizes():
    lib = smml.lib()
    assert lib.smml_fewk_attn_fwd_workspace_bytes(3, 300, 4, 256, 7) == 0                                    # no sum crosses rows
    assert lib.smml_fewk_attn_bwd_workspace_bytes(3, 300, 4, 256, 256, 7) == 3 * 7 * 4 * (256 + 256 + 4) * 4
    assert lib.smml_fewk_attn_bwd_workspace_bytes(2, 300, 8, 512, 256, 300) == 2 * 300 * 8 * (512 + 256 + 4) * 4
    assert lib.smml_fewk_attn_bwd_workspace_bytes(8, 10000, 4, 256, 256, 0) == 8 * 125 * 4 * (256 + 256 + 4) * 4   # 128 wanted: 79 rows, 80 in whole tiles
    assert lib.smml_fewk_attn_bwd_workspace_bytes(2, 11, 4, 256, 256, 0) == 2 * 1 * 4 * (256 + 256 + 4) * 4       # never under 64 rows
    assert lib.smml_fewk_attn_bwd_workspace_bytes(0, 11, 4, 256, 256, 0) == 0


def folded(q, k, v, p, kpm=None):
    """The few-key folded form in plain torch, as MultiheadAttention._forward_few_key composes it around the core: the projections of
    the queries and of the output never touch the bag."""
    E = q.shape[-1]
    w, b = p["in_proj_weight"], p["in_proj_bias"]
    s = E ** -0.5
    kh = k.transpose(0, 1) @ w[E:2 * E].t() + b[E:2 * E]                 # [B, S, E]
    vh = v.transpose(0, 1) @ w[2 * E:].t() + b[2 * E:]
    u, c = s * (kh @ w[:E]), s * (kh @ b[:E])                            # u_j = s Wq^T k^_j, c_j = s bq . k^_j
    wj = vh @ p["out_proj.weight"].t() + p["out_proj.bias"]              # w_j = Wo v^_j + bo
    raw = q.transpose(0, 1) @ u.transpose(1, 2) + c[:, None, :]          # [B, L, S]
    if kpm is not None:
        raw = raw.masked_fill(kpm[:, None, :], float("-inf"))
    return (torch.softmax(raw, -1) @ wj).transpose(0, 1), raw[:, None]


@pytest.mark.parametrize("variant", ["masked", "k is v"])
def test_folded_form_is_the_oracle_in_fp64(variant):
    """The written record of the algebra the kernels rely on (`folded` above against the oracle: outputs, dq, dk, dv and the four parameter
    gradients).  It runs no project code and holds on any revision; the GPU file tests the kernels against the same oracle."""
    L, S, B, E = 50, 4, 2, 64
    g = torch.Generator().manual_seed(6)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)          # noqa: E731
    p = {"in_proj_weight": rnd(3 * E, E) / 8, "in_proj_bias": rnd(3 * E), "out_proj.weight": rnd(E, E) / 8, "out_proj.bias": rnd(E)}
    q, k, v = rnd(L, B, E), rnd(S, B, E), rnd(S, B, E)
    wo, wr = rnd(L, B, E), rnd(B, 1, L, S)
    kpm = None
    if variant == "masked":
        kpm = torch.zeros(B, S, dtype=torch.bool); kpm[0, 1] = True; kpm[1, 3] = True
    res = []
    for fn in (lambda a, b_, c_, d_: coattention(a, b_, c_, d_, key_padding_mask=kpm), lambda a, b_, c_, d_: folded(a, b_, c_, d_, kpm)):
        leaves = [t.clone().requires_grad_() for t in (q, k, v, *p.values())]
        vl = leaves[1] if variant == "k is v" else leaves[2]
        out, raw = fn(leaves[0], leaves[1], vl, dict(zip(p, leaves[3:])))
        fin = torch.isfinite(raw)
        ((out * wo).sum() + (torch.where(fin, raw, torch.zeros_like(raw)) * wr).sum() * 1e-2).backward()
        grads = [t.grad for t in leaves if t is not leaves[2] or variant != "k is v"]
        assert all(gr is not None for gr in grads)
        res.append([out.detach(), torch.where(fin, raw, torch.zeros_like(raw)).detach()] + grads)
        assert int((~fin).sum()) == (L * B if variant == "masked" else 0)
    assert len(res[0]) == (2 + 7 if variant == "masked" else 2 + 6)
    for a, b_ in zip(*res):
        assert float((a - b_).abs().max()) <= 1e-12 * max(1.0, float(b_.abs().max()))
