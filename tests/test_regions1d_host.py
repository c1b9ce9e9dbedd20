"""CPU: the interface of the 1-D position bias per linear piece (csrc/cpb_regions1d.h; include/smml.h "region1d" entry points) -
declared, exported and bound with matching arity; the module / model switches exist with their defaults; every combination the piece
path does not support raises instead of falling back."""
import argparse
import inspect

import pytest
import torch

from helpers import header_arity, smml

Fh = smml.functional
NEW = ("smml_cpb_regions1d_bytes", "smml_cpb_regions1d_build", "smml_deform_attn_region1d_fwd_f32",
       "smml_deform_attn_region1d_bwd_workspace_bytes", "smml_deform_attn_region1d_bwd_f32")


def test_region1d_symbols_declared_exported_and_bound():
    decl = header_arity()
    sig = smml._capi.SIGNATURES
    L = smml.lib()
    for name in NEW:
        assert name in decl, f"{name} is not declared in include/smml.h"
        assert name in sig, f"{name} has no ctypes signature"
        assert len(sig[name][1]) == decl[name], f"{name}: header arity {decl[name]} != SIGNATURES arity {len(sig[name][1])}"
        assert hasattr(L, name), f"{name} is not exported by the library"
    assert L.smml_abi_version() == 2
    assert L.smml_cpb_regions1d_bytes() > 0
    assert L.smml_deform_attn_region1d_bwd_workspace_bytes(8, 10001, 2501, 8) > 0
    assert L.smml_deform_attn_region1d_bwd_workspace_bytes(8, 10001, Fh.REGION_MAX_KEYS + 1, 8) == 0
    # validation before any launch: null pointers and bad arguments are errors with a message
    assert L.smml_cpb_regions1d_build(None, None, None, None, None, None, 2, 1.0, None, 0, None) < 0
    assert L.smml_last_error()
    assert L.smml_deform_attn_region1d_fwd_f32(*([None] * 10), 8, 100, 25, 8, 4, 0.125, 0.0, 0, None, None, None, None) < 0
    assert L.smml_deform_attn_region1d_fwd_f32(*([None] * 10), 8, 100, 25, 8, 2, 0.125, 0.0, 0, None, None, None, None) < 0   # H / G = 4


def test_deform1d_module_takes_cpb_regions_keyword_only():
    p = inspect.signature(smml.DeformCrossAttention1D.__init__).parameters["cpb_regions"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    assert smml.DeformCrossAttention1D(dim=128).cpb_regions is False
    assert smml.DeformCrossAttention1D(dim=128, cpb_regions=True).cpb_regions is True
    for bad in ({"compute_dtype": "bf16"}, {"compute_dtype": "bf16", "cpb_table": True}, {"cpb_log_distance": False}):
        with pytest.raises(ValueError):
            smml.DeformCrossAttention1D(dim=128, cpb_regions=True, **bad)
    layer = inspect.signature(smml.deform_cross_trans_mil.DeformCrossTransLayer.__init__).parameters["cpb_regions_1d"]
    assert layer.default is False


def _args(**kw):
    return argparse.Namespace(path_dim=128, attn_dim=1, input_path_dim=64, **kw)


def test_mil_reads_deform1d_cpb_regions():
    assert smml.DeformCrossTransMIL(_args()).layer3.attn1d.cpb_regions is False
    assert smml.DeformCrossTransMIL(_args(deform1d_cpb_regions=False)).layer3.attn1d.cpb_regions is False
    assert smml.DeformCrossTransMIL(_args(deform1d_cpb_regions=True)).layer3.attn1d.cpb_regions is True
    with pytest.raises(ValueError):
        smml.DeformCrossTransMIL(_args(deform1d_cpb_regions=True, deform_compute_dtype="bf16"))


def _call(heads=8, groups=4, J=25, **kw):
    B, N = 1, 100
    q = torch.zeros(B, N, heads * 64)
    k = v = torch.zeros(B, J, heads * 64)
    vs, gq = torch.zeros(B * groups, J, 1), torch.zeros(N, 1)
    w = [torch.zeros(32, 1), torch.zeros(32), torch.zeros(32, 32), torch.zeros(32), torch.zeros(heads // groups, 32), torch.zeros(heads // groups)]
    return Fh.deform_attention(q, k, v, vs, gq, *w, heads=heads, groups=groups, scale=0.125, cpb_regions=True, **kw)


@pytest.mark.parametrize("kw,what", [({"log_distance": False}, "raw distances"), ({"compute_dtype": "bf16"}, "16-bit"),
                                     ({"compute_dtype": "fp16"}, "16-bit"), ({"compute_dtype": "bf16", "cpb_table": True}, "16-bit"),
                                     ({"compute_dtype": "bf16", "cpb_table": "forward"}, "16-bit"),
                                     ({"heads": 8, "groups": 2}, "heads // groups"), ({"heads": 8, "groups": 1}, "heads // groups"),
                                     ({"J": Fh.REGION_MAX_KEYS + 1}, "keys")])
def test_unsupported_1d_combinations_raise(kw, what):
    """An explicit cpb_regions=True on a 1-D call the piece path cannot take raises (no silent fall-back to the per-pair kernels);
    checked before anything reaches a device."""
    with pytest.raises(ValueError, match=what):
        _call(**kw)
    why = Fh.region1d_unsupported(torch.zeros(4, 25, 1), torch.zeros(1, 25, 512), torch.zeros(32, 32), torch.zeros(2, 32), heads=8, groups=4)
    assert why is None
