"""CPU: the host side of the attention maps (include/smml.h smml_attn_maps_workspace_bytes / smml_attn_maps_f32 / smml_attn_splat_f32;
functional.deform_attention(attn_scores=...), deform_attention_maps; return_attn_maps of the modules, attention_maps of the models):
the symbols are declared, exported and bound; the workspace size neither wraps nor decreases; arguments are validated before any launch;
the options the maps do not support raise ValueError naming them; nothing falls back to the CPU."""
import argparse
import inspect

import pytest
import torch

from helpers import smml

Fh = smml.functional
NEW = ("smml_attn_maps_workspace_bytes", "smml_attn_maps_f32", "smml_attn_splat_f32")


def test_symbols_declared_exported_and_bound():
    L = smml.lib()
    for name in NEW:
        assert name in smml.SIGNATURES, f"{name} is missing from _capi.SIGNATURES"
        assert hasattr(L, name), f"{name} is not exported by the library"
    assert L.smml_abi_version() == 2


def test_workspace_bytes_do_not_wrap_and_are_monotone():
    f = smml.lib().smml_attn_maps_workspace_bytes
    for s in [(0, 0, 0, 0), (-1, 5, 5, 8), (1, 0, 1, 1), (1, 1, -3, 1), (1, 1, 1, 0), (-2147483648, 1, 1, 1)]:
        assert f(*s) == 0, s
    # partial rows [B, H, ceil(ceil(N / 32) / 8), J] fp32 (include/smml.h)
    expect = lambda B, N, J, H: B * H * (((N + 31) // 32 + 7) // 8) * J * 4
    shapes = [(1, 1, 1, 1), (8, 10000, 625, 8), (1, 50176, 3136, 8), (64, 50176, 768, 8), (65535, 1, 1, 1), (1, 2147483647, 1, 1),
              (8, 1 << 20, 768, 8), (1, 1, 2147483647, 8)]
    for s in shapes:
        assert f(*s) == expect(*s), s
    assert f(8, 10000, 625, 8) == 8 * 8 * 40 * 625 * 4
    top = 2 ** 64 - 1
    assert f(2147483647, 2147483647, 2147483647, 2147483647) == top, "a size beyond size_t must saturate, not wrap"
    for base in shapes + [(2147483647, 2147483647, 2147483647, 2147483647)]:
        for i in range(4):
            prev = 0
            for x in (1, 2, 31, 32, 33, 255, 256, 257, 10000, 1 << 20, 2147483647):
                s = list(base)
                s[i] = x
                cur = f(*s)
                assert cur >= prev, f"not monotone in argument {i}: {s} -> {cur} < {prev}"
                prev = cur


def test_null_and_bad_arguments_are_errors_not_launches():
    L = smml.lib()
    assert L.smml_attn_maps_f32(None, None, None, None, None, 0, 0, 0, 0, 0, None) < 0
    assert L.smml_attn_maps_f32(None, None, None, None, None, 1 << 20, 8, 8, 8, 8, None) < 0 and b"null" in L.smml_last_error()
    assert L.smml_attn_maps_f32(None, None, None, None, None, 1 << 20, 8, 1 << 27, 8, 8, None) < 0 and b"2^26" in L.smml_last_error()
    assert L.smml_attn_splat_f32(None, None, None, 0, 0, 0, 0, 0, 0, None) < 0
    assert L.smml_attn_splat_f32(None, None, None, 8, 8, 8, 8, 8, 8, None) < 0 and b"null" in L.smml_last_error()
    assert L.smml_attn_splat_f32(None, None, None, 8, 8, 3, 8, 8, 8, None) < 0 and b"divisible" in L.smml_last_error()


def _core_args(PD=2, W=32, H=8, G=8, B=1, N=40, J=9):
    o = H // G
    return (torch.randn(B, N, H * 64), torch.randn(B, J, H * 64), torch.randn(B, J, H * 64), torch.rand(B * G, J, PD), torch.rand(N, PD),
            torch.randn(W, PD), torch.randn(W), torch.randn(W, W), torch.randn(W), torch.randn(o, W), torch.randn(o))


@pytest.mark.parametrize("kw,word", [({"compute_dtype": "bf16"}, "compute_dtype"), ({"compute_dtype": "fp16"}, "compute_dtype"),
                                     ({"compute_dtype": "bf16", "cpb_table": True}, "cpb_table"),
                                     ({"compute_dtype": "fp16", "cpb_table": "forward"}, "cpb_table")])
def test_unsupported_options_raise_value_error_naming_them(kw, word):
    with pytest.raises(ValueError, match=word):
        Fh.deform_attention(*_core_args(), heads=8, groups=8, scale=0.125, attn_scores=Fh.AttnScores(), **kw)
    for cls, n in ((smml.DeformCrossAttention2D, 144), (smml.DeformCrossAttention1D, 70)):
        mod = cls(dim=128, **kw).eval()
        with pytest.raises(ValueError, match=word):
            mod.forward_tokens(torch.randn(1, n, 128), torch.randn(1, n, 128), return_attn_maps=True)


def test_maps_function_refuses_what_it_cannot_read():
    with pytest.raises(ValueError, match="no scores"):
        Fh.deform_attention_maps(Fh.AttnScores(), heads=8, groups=8)
    nst = smml.lib().smml_deform_attn_nst(40)
    with pytest.raises(ValueError, match="compute_dtype"):
        Fh.deform_attention_maps((torch.zeros(1, 8, nst // 32, 9, 32, dtype=torch.float16), torch.zeros(1, 8, 40)), heads=8, groups=8)
    with pytest.raises(ValueError, match="heads"):
        Fh.deform_attention_maps((torch.zeros(1, 8, nst // 32, 9, 32), torch.zeros(1, 8, 40)), heads=4, groups=4)
    with pytest.raises(TypeError):
        Fh.deform_attention(*_core_args(), heads=8, groups=8, scale=0.125, attn_scores=[])
    with pytest.raises(ValueError, match="return_attn_maps"):
        smml.DeformCrossAttention2D(dim=128).forward_tokens(torch.randn(1, 144, 128), torch.randn(1, 144, 128), return_attn_maps="all")


def test_no_cpu_fallback():
    """CPU tensors raise as before, with or without maps: the product path has no CPU or eager form."""
    for cls, n in ((smml.DeformCrossAttention2D, 144), (smml.DeformCrossAttention1D, 70)):
        mod = cls(dim=128).eval()
        for kw in ({}, {"return_attn_maps": True}, {"return_attn_maps": "dense"}):
            with pytest.raises(RuntimeError, match="GPU|HBM|CPU"):
                mod(torch.randn(1, 128, n), torch.randn(1, 128, n), **kw)
    with pytest.raises(RuntimeError, match="GPU|HBM|CPU"):
        Fh.deform_attention_maps((torch.zeros(1, 8, 4, 9, 32), torch.zeros(1, 8, 40)), heads=8, groups=8)


def test_interfaces_are_additive():
    for cls in (smml.DeformCrossAttention2D, smml.DeformCrossAttention1D):
        assert list(inspect.signature(cls.forward).parameters)[1:] == ["x1", "x2", "return_vgrid"]          # the reference's, as reported
        with pytest.raises(ValueError, match="return_attn_maps"):                                           # ... and the keyword is taken
            cls(dim=128)(torch.randn(1, 128, 144), torch.randn(1, 128, 144), return_attn_maps="all")
        p = inspect.signature(cls.forward_tokens).parameters
        assert list(p)[1:5] == ["x1t", "x2t", "return_vgrid", "residual"] and p["return_attn_maps"].default is False
    assert inspect.signature(Fh.deform_attention).parameters["attn_scores"].default is None
    assert list(inspect.signature(smml.DeformCrossTransMIL.forward).parameters)[1:] == ["path", "omic"]
    assert list(inspect.signature(smml.DeformCrossTransMIL.attention_maps).parameters)[1:3] == ["path", "omic"]
    assert "_maps_out" not in smml.DeformCrossTransMIL(argparse.Namespace(path_dim=128, input_path_dim=64, attn_dim=2, return_vgrid=False)).state_dict()


def test_models_need_the_2d_branch():
    net = smml.DeformCrossTransMIL(argparse.Namespace(path_dim=128, input_path_dim=64, attn_dim=1, return_vgrid=False)).eval()
    with pytest.raises(ValueError, match="attn_dim"):
        net.attention_maps(torch.randn(1, 144, 64), torch.randn(1, 128))
    assert net._maps_out is None
    from test_oracle_golden import pathomic_args
    pn = smml.DeformPathomicNet(pathomic_args(attn_dim=1, return_vgrid=False)).eval()
    with pytest.raises(ValueError, match="attn_dim"):
        pn.attention_maps(x_path=torch.randn(1, 144, 1024), x_omic_tumor=torch.randn(1, 59), x_omic_immune=torch.randn(1, 361))
