"""CPU: MCAT_Surv without a device - the fp32 / fp64 oracle tests/mcat_oracle.py against the reference's fixture tests/golden/mcat_n150.npz
(tests/golden/make_golden_mcat.py), the interfaces of smml.MCAT_Surv and its parts (parameter names, shapes and order, signatures,
checkpoints exchanged with torch.nn's encoder), the C-ABI entries of the token-set kernels (csrc/token_set.hip), functional.token_why and
the shape errors of the two functionals and of the entry points themselves, which are raised before anything is launched."""
import argparse
import ctypes
import inspect

import pytest
import torch

import mcat_oracle as mo
from helpers import Golden, assert_zero_grad, header_arity, smml

Fh = smml.functional
TOKEN_SYMBOLS = {"smml_token_attn_fwd_f32": 14, "smml_token_attn_bwd_f32": 17, "smml_token_pool_gated_fwd_f32": 14,
                 "smml_token_pool_gated_bwd_f32": 18}
STORED = ("logits", "hazards", "S", "A_coattn", "A_path", "A_omic", "dx_path", "dx_omic")


def check_against_fixture(g, res):
    """The fixture's rules for one evaluation `res` (mcat_oracle.run's table, or the same keys from the HIP module)."""
    for k in STORED:
        g.check(k, res[k])
    assert abs(res["loss"] - g.scalar("loss")) <= 1e-4 * abs(g.scalar("loss"))
    for k in mo.PARAMS:
        if k in mo.ZERO_GRADS:
            assert_zero_grad(f"{g.name}:d{k}", res["grad:" + k], g.scalar("natural:" + k))
        else:
            g.check("grad:" + k, res["grad:" + k], what="d" + k)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_oracle_matches_reference(dtype):
    g = Golden("mcat_n150")
    res = mo.run(*mo.problem(2, 150), dtype)
    check_against_fixture(g, res)
    assert tuple(res["A_coattn"].shape) == (2, 1, 4, 150) and tuple(res["A_path"].shape) == tuple(res["A_omic"].shape) == (2, 1, 4)
    for k in mo.ZERO_GRADS:
        assert abs(res["natural:" + k] - g.scalar("natural:" + k)) <= 1e-3 * res["natural:" + k]
    assert all(float(res["grad:" + k].abs().max()) > 0 for k in mo.PARAMS if k not in mo.ZERO_GRADS), "every parameter receives a gradient"


def test_parameter_names_shapes_and_order_are_the_reference_s():
    g = Golden("mcat_n150")
    stored = {str(n): tuple(int(d) for d in str(s).split(",")) for n, s in zip(g.array("param_names"), g.array("param_shapes"))}
    mod = smml.MCAT_Surv(argparse.Namespace(label_dim=4))
    assert len(stored) == 92
    assert {k: tuple(v.shape) for k, v in mod.state_dict().items()} == stored == mo.PARAMS
    assert list(mod.state_dict()) == [str(n) for n in g.array("param_names")] == list(mo.PARAMS)
    mod.load_state_dict(mo.problem(1, 1)[2], strict=True)
    assert mod.mcat_fused and mod.coattn.fused_few_query and all(l.fused for l in mod.path_transformer.layers)
    off = smml.MCAT_Surv(argparse.Namespace(label_dim=4, mcat_fused=False))
    assert not off.mcat_fused and not off.coattn.fused_few_query and not any(l.fused for l in off.omic_transformer.layers)
    assert list(off.state_dict()) == list(mod.state_dict())
    assert smml.MCAT_Surv(argparse.Namespace(label_dim=3)).classifier.weight.shape == (3, 256)
    bil = smml.MCAT_Surv(argparse.Namespace(label_dim=4), fusion="bilinear")
    assert type(bil.mm) is smml.BilinearFusion


def test_signatures_are_the_reference_s():
    sig = inspect.signature(smml.MCAT_Surv.__init__).parameters
    assert list(sig) == ["self", "args", "fusion", "omic_sizes", "n_classes", "model_size_wsi", "model_size_omic", "dropout"]
    assert (sig["fusion"].default, sig["omic_sizes"].default, sig["n_classes"].default, sig["model_size_wsi"].default,
            sig["model_size_omic"].default, sig["dropout"].default) == ("concat", [100, 100, 100, 131], 4, "small", "small", 0.25)
    fwd = inspect.signature(smml.MCAT_Surv.forward).parameters
    assert list(fwd) == ["self", "kwargs"] and fwd["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    head = inspect.signature(smml.Attn_Net_Gated.__init__).parameters
    assert list(head) == ["self", "L", "D", "dropout", "n_classes"] and (head["L"].default, head["D"].default) == (1024, 256)
    assert list(smml.Attn_Net_Gated(256, 256, 0.25).state_dict()) == ["attention_a.0.weight", "attention_a.0.bias", "attention_b.0.weight",
                                                                        "attention_b.0.bias", "attention_c.weight", "attention_c.bias"]
    for name in ("MCAT_Surv", "Attn_Net_Gated", "TransformerEncoder", "TransformerEncoderLayer"):
        assert name in smml.__all__ and hasattr(smml, name)


def test_encoder_checkpoints_load_in_both_directions():
    ours = smml.TransformerEncoder(smml.TransformerEncoderLayer(d_model=256, nhead=8, dim_feedforward=512, dropout=0.25, activation="relu"), 2)
    theirs = torch.nn.TransformerEncoder(torch.nn.TransformerEncoderLayer(d_model=256, nhead=8, dim_feedforward=512, dropout=0.25,
                                                                          activation="relu"), num_layers=2)
    assert list(ours.state_dict()) == list(theirs.state_dict())
    assert {k: v.shape for k, v in ours.state_dict().items()} == {k: v.shape for k, v in theirs.state_dict().items()}
    theirs.load_state_dict(ours.state_dict(), strict=True)
    ours.load_state_dict(theirs.state_dict(), strict=True)
    assert ours.layers[0].self_attn.in_proj_weight is not ours.layers[1].self_attn.in_proj_weight          # deep copies, as torch.nn's
    with pytest.raises(NotImplementedError):
        smml.TransformerEncoderLayer(256, 8, activation="gelu")


def test_token_entries_are_declared_exported_and_bound():
    arity = header_arity()
    lib = smml.lib()
    for name, n in TOKEN_SYMBOLS.items():
        assert name in smml.SIGNATURES and hasattr(lib, name), name
        assert len(smml.SIGNATURES[name][1]) == arity[name] == n, name
        assert len(smml._capi.PARAMS[name]) == n
    assert smml._capi.ABI_VERSION == 2 == lib.smml_abi_version()
    # the launches go by name: each key set is exactly its prototype's parameter names
    for name, keys in (("smml_token_attn_fwd_f32", Fh.TOKEN_ATTN_FWD_KEYS), ("smml_token_attn_bwd_f32", Fh.TOKEN_ATTN_BWD_KEYS),
                       ("smml_token_pool_gated_fwd_f32", Fh.TOKEN_POOL_FWD_KEYS), ("smml_token_pool_gated_bwd_f32", Fh.TOKEN_POOL_BWD_KEYS)):
        assert {p for p, _, _ in smml._capi.PARAMS[name]} == keys, name


@pytest.mark.parametrize("kw, what", [(dict(T=9, E=256, heads=8), "9 tokens"), (dict(T=0, E=256, heads=8), "0 tokens"),
                                      (dict(T=4, E=100, heads=4), "token width 100"), (dict(T=4, E=576, heads=9), "token width 576"),
                                      (dict(T=4, E=256, heads=16), "head dim 256/16"), (dict(T=4, E=256, heads=2), "head dim 256/2"),
                                      (dict(T=4, E=192, heads=5), "head dim 192/5"), (dict(T=4, E=256, heads=8, attn_mask=True), "attention mask"),
                                      (dict(T=4, E=256, heads=8, key_padding_mask=True), "key padding mask"),
                                      (dict(T=4, E=256, heads=8, fused=False), "switched off"), (dict(T=4, E=256, D=96), "96 hidden units"),
                                      (dict(T=4, E=256, D=320), "320 hidden units"), (dict(T=9, E=256, D=256), "9 tokens")])
def test_token_why_names_each_unsupported_combination(kw, what):
    assert what in Fh.token_why(**kw) and Fh.token_path(**kw) == "composed"


def test_token_why_accepts_what_the_kernels_take():
    for kw in (dict(T=4, E=256, heads=8), dict(T=8, E=512, heads=8), dict(T=1, E=64, heads=2), dict(T=3, E=192, heads=6), dict(T=8, E=64, heads=1),
               dict(T=4, E=256, D=256), dict(T=1, E=256, D=64), dict(T=8, E=512, D=128)):
        assert Fh.token_why(**kw) is None and Fh.token_path(**kw) == "token"


@pytest.mark.parametrize("shape, heads, what", [((2, 9, 768), 8, "9 tokens"), ((2, 4, 300), 4, "token width 100"), ((2, 4, 768), 16, "head dim"),
                                                ((2, 4, 767), 8, "packed projection")], ids=["T9", "E100", "hd16", "not-3E"])
def test_self_attention_refuses_before_any_launch(shape, heads, what):
    with pytest.raises(ValueError, match=what):          # CPU tensors: reaching a launch would raise RuntimeError instead
        Fh.token_self_attention(torch.zeros(shape), heads=heads)


def test_pooling_refuses_before_any_launch():
    w, b = torch.zeros(1, 256), torch.zeros(1)
    with pytest.raises(ValueError, match="9 tokens"):
        Fh.token_pool_gated(torch.zeros(2, 9, 256), torch.zeros(2, 9, 512), w, b)
    with pytest.raises(ValueError, match="token width 100"):
        Fh.token_pool_gated(torch.zeros(2, 4, 100), torch.zeros(2, 4, 512), w, b)
    with pytest.raises(ValueError, match="96 hidden units"):
        Fh.token_pool_gated(torch.zeros(2, 4, 256), torch.zeros(2, 4, 192), torch.zeros(1, 96), b)
    with pytest.raises(ValueError, match="same tokens"):
        Fh.token_pool_gated(torch.zeros(2, 4, 256), torch.zeros(2, 5, 512), w, b)
    with pytest.raises(ValueError, match="one attention map"):
        Fh.token_pool_gated(torch.zeros(2, 4, 256), torch.zeros(2, 4, 512), torch.zeros(2, 256), b)
    with pytest.raises(ValueError, match="keep must be"):
        Fh.token_self_attention(torch.zeros(2, 4, 768), heads=8, keep=torch.ones(2, 8, 4, 5))


def test_entry_points_refuse_before_any_launch():
    """The C entry points themselves: T = 9, E = 100, hd = 16 and D = 96 return an error code and a message; the pointers are never
    dereferenced on the host and no kernel is launched (validation comes first)."""
    lib = smml.lib()
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    attn = lambda T, E, H: lib.smml_token_attn_fwd_f32(ptr, None, ptr, ptr, 2, T, E, H, 3 * E * T, 3 * E, E * T, E, 0.125, None)      # noqa: E731
    attn_b = lambda T, E, H: lib.smml_token_attn_bwd_f32(ptr, None, ptr, ptr, ptr, 2, T, E, H, 3 * E * T, 3 * E, E * T, E, 3 * E * T, 3 * E,      # noqa: E731
                                                         0.125, None)
    pool = lambda T, E, D: lib.smml_token_pool_gated_fwd_f32(ptr, ptr, ptr, ptr, ptr, ptr, ptr, 2, T, E, D, E * T, E, None)      # noqa: E731
    pool_b = lambda T, E, D: lib.smml_token_pool_gated_bwd_f32(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, 2, T, E, D, E * T, E, E * T, E, None)      # noqa: E731
    for fn, name in ((attn, "smml_token_attn_fwd_f32"), (attn_b, "smml_token_attn_bwd_f32")):
        for T, E, H in ((9, 256, 8), (4, 100, 4), (4, 256, 16), (0, 256, 8)):
            assert fn(T, E, H) == -1, (name, T, E, H)
            assert name in lib.smml_last_error().decode()
    for fn, name in ((pool, "smml_token_pool_gated_fwd_f32"), (pool_b, "smml_token_pool_gated_bwd_f32")):
        for T, E, D in ((9, 256, 256), (4, 100, 256), (4, 256, 96), (4, 256, 320)):
            assert fn(T, E, D) == -1, (name, T, E, D)
            assert name in lib.smml_last_error().decode()
    # strides that are no multiple of four floats, or rows that overlap
    assert lib.smml_token_attn_fwd_f32(ptr, None, ptr, ptr, 2, 4, 256, 8, 3072, 770, 1024, 256, 0.125, None) == -1
    assert lib.smml_token_attn_fwd_f32(ptr, None, ptr, ptr, 2, 4, 256, 8, 3072, 256, 1024, 256, 0.125, None) == -1
    assert lib.smml_token_pool_gated_fwd_f32(None, ptr, ptr, ptr, ptr, ptr, ptr, 2, 4, 256, 256, 1024, 256, None) == -1
