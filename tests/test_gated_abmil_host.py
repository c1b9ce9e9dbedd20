"""CPU: the gated attention-pooling baseline without a device - the fp32 / fp64 oracle tests/gated_abmil_oracle.py against the reference's
fixture tests/golden/gated_abmil_n300.npz (tests/golden/make_golden_gated_abmil.py), the interfaces of smml.GatedABMIL and of ABMIL with
the extension key `abmil_gated` (parameter names, shapes and order, signatures, define_net's modes), the C-ABI entries of the gated
pooling kernels, and the shape errors of functional.attention_pool_gated and of linear's halves epilogue, which are raised before
anything is launched."""
import inspect

import pytest
import torch

import gated_abmil_oracle as go
from helpers import Golden, assert_zero_grad, header_arity, smml
from test_abmil_host import net_args

Fh = smml.functional
GATED_SYMBOLS = {"smml_attn_pool_gated_fwd_f32": 15, "smml_attn_pool_gated_bwd_f32": 18}
PLAIN_KEYS = ["attention.0.weight", "attention.0.bias", "attention.2.weight", "attention.2.bias", "classifier.0.weight", "classifier.0.bias",
              "multimodal_projection.weight", "multimodal_projection.bias"]          # ABMIL's state_dict before the extension key existed


def check_against_fixture(g, res):
    """The fixture's rules for one evaluation `res` (gated_abmil_oracle.run_reference's table, or the same keys from the HIP module)."""
    g.check("prob", res["prob"]); g.check("softmax", res["softmax"])
    assert abs(res["loss"] - g.scalar("loss")) <= 1e-4 * abs(g.scalar("loss"))
    for k in go.PARAMS:
        if k == go.ZERO_GRAD:
            assert_zero_grad(f"{g.name}:d{k}", res["grad:" + k], g.scalar("natural:" + k))
        else:
            g.check("grad:" + k, res["grad:" + k], what="d" + k)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_oracle_matches_reference(dtype):
    g = Golden("gated_abmil_n300")
    res = go.run_reference(*go.reference_problem(300), dtype)
    check_against_fixture(g, res)
    assert tuple(res["softmax"].shape) == (1, 1, 300) and tuple(res["prob"].shape) == (1, 2)
    assert abs(res["natural"] - g.scalar("natural:" + go.ZERO_GRAD)) <= 1e-4 * res["natural"]
    assert float(res["grad:attention_U.0.weight"].abs().max()) > 0 and float(res["grad:attention_V.0.weight"].abs().max()) > 0


def test_parameter_names_shapes_and_order_are_the_reference_s():
    g = Golden("gated_abmil_n300")
    stored = {str(n): tuple(int(d) for d in str(s).split(",")) for n, s in zip(g.array("param_names"), g.array("param_shapes"))}
    mod = smml.GatedABMIL()
    assert {k: tuple(v.shape) for k, v in mod.state_dict().items()} == stored == go.PARAMS
    assert list(mod.state_dict()) == [str(n) for n in g.array("param_names")] == list(go.PARAMS)
    assert (mod.L, mod.D, mod.K) == (1024, 128, 1) and mod.pool_splits is None
    mod.load_state_dict(go.reference_problem(1)[1], strict=True)
    assert list(inspect.signature(smml.GatedABMIL.forward).parameters) == ["self", "x", "subtype_labels", "adj", "mask"]
    assert list(inspect.signature(smml.GatedABMIL.__init__).parameters) == ["self"]
    assert "GatedABMIL" in smml.__all__


def test_abmil_without_the_key_is_unchanged():
    for args in (net_args(), net_args(abmil_gated=False)):
        mod = smml.ABMIL(args)
        assert list(mod.state_dict()) == PLAIN_KEYS
        assert not hasattr(mod, "attention_V") and not hasattr(mod, "attention_out")


def test_abmil_with_the_key_has_the_gated_parameters():
    mod = smml.ABMIL(net_args(abmil_gated=True))
    assert {k: tuple(v.shape) for k, v in mod.state_dict().items()} == go.NET_PARAMS
    assert list(mod.state_dict()) == list(go.NET_PARAMS)
    assert not hasattr(mod, "attention") and callable(mod.attention_weights)
    mod.load_state_dict(go.problem(1, 1)[1], strict=True)
    assert list(inspect.signature(mod.forward).parameters) == ["x"]


def test_define_net_with_the_key():
    net = smml.define_net(net_args(mode="path", abmil_gated=True))
    assert type(net) is smml.ABMIL and list(net.state_dict()) == list(go.NET_PARAMS)
    assert list(smml.define_net(net_args(mode="path")).state_dict()) == PLAIN_KEYS
    for mode in ("mcat", "pathomic", "pathomic_original"):
        with pytest.raises(NotImplementedError):
            smml.define_net(net_args(mode=mode, abmil_gated=True))


def test_gated_pool_entries_are_declared():
    arity = header_arity()
    for name, n in GATED_SYMBOLS.items():
        assert name in smml.SIGNATURES, name
        assert len(smml.SIGNATURES[name][1]) == arity[name] == n, name
    assert smml._capi.ABI_VERSION == 2
    assert (Fh.ACT_NONE, Fh.ACT_RELU, Fh.ACT_TANH, Fh.ACT_SIGMOID, Fh.ACT_TANH_SIGMOID) == (0, 1, 2, 3, 4)


@pytest.mark.parametrize("L, W, wn, what", [(1024, 255, 127, "2 D"), (1024, 192, 96, "2 D"), (1024, 640, 320, "2 D"), (896, 256, 128, "feature width"),
                                            (1024, 256, 64, "K = 1"), (1024, 256, 256, "K = 1")],
                         ids=["h2-odd", "h2-not-128k", "h2-above-512", "L-896", "w-half", "w-double"])
def test_bad_shapes_raise_before_any_launch(L, W, wn, what):
    x, h2 = torch.zeros(2, 5, L), torch.zeros(2, 5, W)          # CPU tensors: reaching a launch would raise RuntimeError instead
    with pytest.raises(ValueError, match=what):
        Fh.attention_pool_gated(x, h2, torch.zeros(1, wn), torch.zeros(1))


def test_other_shape_errors():
    with pytest.raises(ValueError, match="same bag"):
        Fh.attention_pool_gated(torch.zeros(2, 5, 1024), torch.zeros(2, 6, 256), torch.zeros(1, 128), torch.zeros(1))
    with pytest.raises(ValueError, match="K = 1"):
        Fh.attention_pool_gated(torch.zeros(2, 5, 1024), torch.zeros(2, 5, 256), torch.zeros(1, 128), torch.zeros(2))
    with pytest.raises(ValueError, match="outside the autograd graph"):
        Fh.attention_pool_gated(torch.zeros(2, 5, 1024), torch.zeros(2, 5, 256, requires_grad=True), torch.zeros(1, 128), torch.zeros(1),
                                hidden=(torch.zeros(128, 1024), torch.zeros(128), torch.zeros(128, 1024), torch.zeros(128)))


def test_halves_epilogue_needs_an_even_width():
    with pytest.raises(ValueError, match="odd N"):
        Fh.linear(torch.zeros(4, 96), torch.zeros(127, 96), torch.zeros(127), act=Fh.ACT_TANH_SIGMOID)
