"""CPU: the ABMIL baseline (mode 'path' of define_net) without a device - the fp32 / fp64 oracle tests/abmil_oracle.py against the
reference's fixture tests/golden/abmil_n300.npz (tests/golden/make_golden_abmil.py), the module's interface (parameter names and shapes,
forward signature, define_net's modes), the four C-ABI entries of the pooling kernels, and the shape errors of functional.attention_pool,
which are raised before anything is launched."""
import argparse
import inspect

import pytest
import torch

import abmil_oracle as ao
from helpers import Golden, assert_zero_grad, header_arity, smml

Fh = smml.functional
POOL_SYMBOLS = {"smml_attn_pool_fwd_workspace_bytes": 4, "smml_attn_pool_fwd_f32": 15, "smml_attn_pool_bwd_workspace_bytes": 4,
                "smml_attn_pool_bwd_f32": 18}


def net_args(**over):
    a = argparse.Namespace(mode="path", label_dim=3, path_dim=128, init_type="max", input_size_omic=431, omic_dim=128, return_grad="False",
                           dropout_rate=0.1)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def check_against_fixture(g, res):
    """The fixture's rules for one evaluation `res` (abmil_oracle.run's table, or the same keys from the HIP module)."""
    g.check("encoded", res["encoded"]); g.check("logits", res["logits"]); g.check("softmax", res["softmax"])
    assert abs(res["loss"] - g.scalar("loss")) <= 1e-4 * abs(g.scalar("loss"))
    for k in ao.PARAMS:
        if k == ao.ZERO_GRAD:
            assert_zero_grad(f"{g.name}:d{k}", res["grad:" + k], g.scalar("natural:" + k))
        else:
            g.check("grad:" + k, res["grad:" + k], what="d" + k)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_oracle_matches_reference(dtype):
    g = Golden("abmil_n300")
    res = ao.run(*ao.problem(2, 300), dtype)
    check_against_fixture(g, res)
    assert tuple(res["softmax"].shape) == (2, 1, 300)
    assert abs(res["natural"] - g.scalar("natural:" + ao.ZERO_GRAD)) <= 1e-4 * res["natural"]


def test_parameter_names_and_shapes_are_the_reference_s():
    g = Golden("abmil_n300")
    stored = {str(n): tuple(int(d) for d in str(s).split(",")) for n, s in zip(g.array("param_names"), g.array("param_shapes"))}
    mod = smml.ABMIL(net_args())
    assert {k: tuple(v.shape) for k, v in mod.state_dict().items()} == stored == ao.PARAMS
    assert list(mod.state_dict()) == [str(n) for n in g.array("param_names")]
    assert (mod.L, mod.D, mod.K) == (1024, 128, 1)
    mod.load_state_dict(ao.problem(1, 1)[1], strict=True)
    assert list(inspect.signature(smml.ABMIL.forward).parameters) == ["self", "x"]
    assert list(inspect.signature(smml.ABMIL.__init__).parameters) == ["self", "args"]


def test_define_net_modes():
    assert type(smml.define_net(net_args(mode="path"))) is smml.ABMIL
    omic = smml.define_net(net_args(mode="omic"))
    assert type(omic) is smml.MaxNet
    assert tuple(omic.encoder[0][0].weight.shape) == (64, 431) and tuple(omic.classifier[0].weight.shape) == (3, 128)
    for mode in ("mcat", "pathomic", "pathomic_original"):
        with pytest.raises(NotImplementedError):
            smml.define_net(net_args(mode=mode))


def test_pool_entries_are_declared():
    arity = header_arity()
    for name, n in POOL_SYMBOLS.items():
        assert name in smml.SIGNATURES, name
        assert len(smml.SIGNATURES[name][1]) == arity[name] == n, name
    assert smml._capi.ABI_VERSION == 2


@pytest.mark.parametrize("L, D, what", [(1000, 128, "feature width"), (1024, 96, "hidden width"), (1280, 128, "feature width"),
                                        (1024, 320, "hidden width")])
def test_unsupported_widths_raise_before_any_launch(L, D, what):
    x, h = torch.zeros(2, 5, L), torch.zeros(2, 5, D)          # CPU tensors: reaching a launch would raise RuntimeError instead
    with pytest.raises(ValueError, match=what):
        Fh.attention_pool(x, h, torch.zeros(1, D), torch.zeros(1))


def test_other_shape_errors():
    with pytest.raises(ValueError, match="same bag"):
        Fh.attention_pool(torch.zeros(2, 5, 1024), torch.zeros(2, 6, 128), torch.zeros(1, 128), torch.zeros(1))
    with pytest.raises(ValueError, match="K = 1"):
        Fh.attention_pool(torch.zeros(2, 5, 1024), torch.zeros(2, 5, 128), torch.zeros(2, 128), torch.zeros(2))
    with pytest.raises(ValueError, match="outside the autograd graph"):
        Fh.attention_pool(torch.zeros(2, 5, 1024), torch.zeros(2, 5, 128, requires_grad=True), torch.zeros(1, 128), torch.zeros(1),
                          hidden=(torch.zeros(128, 1024), torch.zeros(128)))
