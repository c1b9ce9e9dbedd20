"""CPU: the host side of the fused self-normalising encoder stacks (csrc/snn_stack.hip) - the two C-ABI entries and their validation,
functional.snn_why / snn_stack's shape errors (raised before anything is launched), the extension key `snn_fused` of MaxNet, define_net,
DeformPathomicNet, CMTA and MCAT_Surv (off by default: the composed calls never reach snn_stack), unchanged parameter names - and the
three-term AlphaDropout formula of the kernels against torch's own."""
import argparse
import ctypes

import pytest
import torch

from helpers import header_arity, smml
from test_oracle_golden import pathomic_args

Fh, capi = smml.functional, smml._capi
SNN_SYMBOLS = {"smml_snn_stack_fwd_f32": 15, "smml_snn_stack_bwd_f32": 19}
MCAT_WIDTHS = [[100, 256, 256], [100, 256, 256], [100, 256, 256], [131, 256, 256]]
MAXNET_WIDTHS = [[59, 64, 48, 32, 128], [361, 64, 48, 32, 128]]


def test_c_abi_declares_the_two_entries():
    arity = header_arity()
    lib = smml.lib()
    for name, n in SNN_SYMBOLS.items():
        assert name in smml.SIGNATURES and hasattr(lib, name), name
        assert len(smml.SIGNATURES[name][1]) == arity[name] == n, name
    assert capi.ABI_VERSION == 2 == lib.smml_abi_version()
    names = lambda proto: {n for n, _, _ in capi.PARAMS[proto]}          # noqa: E731
    assert Fh.SNN_FWD_KEYS == names("smml_snn_stack_fwd_f32") and Fh.SNN_BWD_KEYS == names("smml_snn_stack_bwd_f32")


def test_supported_groups_take_the_kernels():
    for widths in (MCAT_WIDTHS, MAXNET_WIDTHS, [[1, 1]], [[7, 33, 5, 48]], [[2048, 256, 256, 256, 256]], [[59, 5]] * 8):
        assert Fh.snn_why(widths) is None and Fh.snn_path(widths) == "snn"
    assert Fh.snn_why(MCAT_WIDTHS, rates=[[0.25, 0.25]] * 4, dtypes=[torch.float32] * 16) is None
    assert Fh.snn_keep_numel(8, MCAT_WIDTHS) == 8 * 4 * 512 and Fh.snn_keep_numel(3, MAXNET_WIDTHS) == 3 * 2 * 272


def test_depth_five_stays_composed():
    assert "depth 5" in Fh.snn_why([[59, 64, 48, 32, 32, 16]]) and Fh.snn_path([[59, 64, 48, 32, 32, 16]]) == "composed"


def test_nine_networks_stay_composed():
    assert "9 networks" in Fh.snn_why([[100, 256, 256]] * 9)


def test_width_257_stays_composed():
    assert "width 257" in Fh.snn_why([[100, 256, 256], [100, 257, 256]])


def test_2049_inputs_stay_composed():
    assert "2049 inputs" in Fh.snn_why([[2049, 256]])


def test_unequal_depths_stay_composed():
    assert "unequal depths" in Fh.snn_why([[100, 256, 256], [100, 256]])


def test_unequal_rates_stay_composed():
    assert "unequal dropout rates" in Fh.snn_why(MCAT_WIDTHS, rates=[[0.25, 0.25], [0.25, 0.1], [0.25, 0.25], [0.25, 0.25]])


def test_other_dtypes_stay_composed():
    assert "dtype" in Fh.snn_why(MCAT_WIDTHS, dtypes=[torch.float32, torch.float64])


def _layers(widths):
    return [torch.zeros(n, k) for k, n in zip(widths, widths[1:])], [torch.zeros(n) for n in widths[1:]]


@pytest.mark.parametrize("widths, what", [([[59, 64, 48, 32, 32, 16]], "depth 5"), ([[10, 257]], "width 257"), ([[2049, 4]], "2049 inputs"),
                                          ([[10, 4]] * 9, "9 networks"), ([[10, 4, 4], [10, 4]], "unequal depths")],
                         ids=["depth5", "N257", "K2049", "G9", "depths"])
def test_snn_stack_refuses_before_any_launch(widths, what):
    ws, bs = zip(*(_layers(w) for w in widths))
    with pytest.raises(ValueError, match=what):          # CPU tensors: reaching a launch would raise RuntimeError instead
        Fh.snn_stack([torch.zeros(2, w[0]) for w in widths], list(ws), list(bs))


def test_snn_stack_refuses_inconsistent_arguments():
    ws, bs = _layers([10, 4])
    with pytest.raises(ValueError, match="keep is required"):
        Fh.snn_stack([torch.zeros(2, 10)], [ws], [bs], p=0.25)
    with pytest.raises(ValueError, match="keep is required"):
        Fh.snn_stack([torch.zeros(2, 10)], [ws], [bs], keep=torch.ones(8))
    with pytest.raises(ValueError, match="keep must hold 8"):
        Fh.snn_stack([torch.zeros(2, 10)], [ws], [bs], p=0.25, keep=torch.ones(9))
    with pytest.raises(ValueError, match="do not follow"):
        Fh.snn_stack([torch.zeros(2, 11)], [ws], [bs])
    with pytest.raises(ValueError, match="same B"):
        Fh.snn_stack([torch.zeros(2, 10), torch.zeros(3, 10)], [ws, ws], [bs, bs])
    with pytest.raises(ValueError, match="dtype"):
        Fh.snn_stack([torch.zeros(2, 10)], [[ws[0].double()]], [bs])
    w2, b2 = _layers([10, 5])
    with pytest.raises(ValueError, match="equal last widths"):
        Fh.snn_stack([torch.zeros(2, 10), torch.zeros(2, 10)], [ws, w2], [bs, b2], stacked=True)
    with pytest.raises(RuntimeError):                      # a supported call on CPU tensors reaches the launch path, which has no CPU form
        Fh.snn_stack([torch.zeros(2, 10)], [ws], [bs])


def test_entry_points_refuse_before_any_launch():
    """Null tables, zero networks, depth 0 and 5, a negative or oversized width, a missing keep: an error code and a message; no table
    entry is dereferenced on the device and nothing is launched (validation comes first)."""
    lib = smml.lib()
    U, L, I = ctypes.c_ulonglong, ctypes.c_longlong, ctypes.c_int
    buf = ctypes.create_string_buffer(64)
    dev = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)          # stands for device memory: never read on the host
    addr = (U * 8)(*[dev.value] * 8)
    zeros, strides = (L * 8)(), (L * 8)(*[16] * 8)

    def fwd(widths, G=1, depth=1, B=2, p=0.0, keep=None, x=addr, tab=addr):
        return lib.smml_snn_stack_fwd_f32(x, strides, zeros, tab, tab, (I * len(widths))(*widths), keep, dev, tab, G, depth, B, p, 0, None)

    def bwd(widths, G=1, depth=1, B=2, p=0.0, keep=None, x=addr, tab=addr):
        return lib.smml_snn_stack_bwd_f32(x, strides, zeros, tab, (I * len(widths))(*widths), keep, dev, tab, tab, dev, tab, tab, None, G, depth, B,
                                          p, 0, None)

    for fn, name in ((fwd, "smml_snn_stack_fwd_f32"), (bwd, "smml_snn_stack_bwd_f32")):
        for kw in (dict(widths=[4, 4], x=None), dict(widths=[4, 4], tab=None), dict(widths=[4, 4], G=0), dict(widths=[4, 4], G=9),
                   dict(widths=[4, 4], depth=0), dict(widths=[4] * 6, depth=5), dict(widths=[4, -1]), dict(widths=[4, 257]),
                   dict(widths=[2049, 4]), dict(widths=[0, 4]), dict(widths=[4, 4], B=0), dict(widths=[4, 4], p=0.25), dict(widths=[4, 4], keep=dev),
                   dict(widths=[4, 4], p=1.0, keep=dev), dict(widths=[4, 4], x=(U * 8)())):
            assert fn(**kw) == -1, (name, kw)
            assert name in lib.smml_last_error().decode(), (name, kw)


def test_alpha_dropout_formula_is_torch_s():
    """The three-term form the kernels and the tests' restatement use, A keep e + A alpha' (keep - 1) + A alpha' p: with keep all ones it
    must give A e + A alpha' p, and with the mask torch drew it must give torch's own output."""
    p, al = 0.25, Fh.SNN_ALPHA
    A = ((al * al * p + 1) * (1 - p)) ** -0.5
    e = torch.linspace(-1, 3, 4001, dtype=torch.float64)
    form = lambda keep: A * keep * e + A * al * (keep - 1) + A * al * p          # noqa: E731
    assert torch.allclose(form(torch.ones_like(e)), A * e + A * al * p, rtol=0, atol=1e-15)
    torch.manual_seed(3)
    out = torch.nn.functional.alpha_dropout(e, p, training=True)
    dropped = A * al * (p - 1)                                                    # where torch dropped, the output is this constant
    keep = ((out - dropped).abs() > 1e-9).double()
    assert 0.7 < float(keep.mean()) < 0.8
    assert torch.allclose(form(keep), out, rtol=0, atol=1e-12)
    assert abs(-al - torch.nn.functional.selu(torch.tensor(-1e4, dtype=torch.float64)).item()) < 1e-12          # alpha' = -selu(-inf)


def _raise(*a, **k):
    raise AssertionError("snn_stack reached without the key")


def _linear_stub(x, w, b=None, **k):
    return torch.nn.functional.linear(x, w, b)


def test_maxnet_without_the_key_never_reaches_snn_stack(monkeypatch):
    monkeypatch.setattr(Fh, "snn_stack", _raise)
    monkeypatch.setattr(Fh, "linear", _linear_stub)          # the composed form's launches, on the CPU
    net = smml.MaxNet(input_dim=59, omic_dim=32, label_dim=4).eval()
    assert net.fused is False
    feats, logits, _ = net(x_omic=torch.randn(3, 59))
    assert tuple(feats.shape) == (3, 32) and tuple(logits.shape) == (3, 4) and float(feats.detach().min()) >= 0
    off = smml.define_net(pathomic_args(mode="omic"))
    assert isinstance(off, smml.MaxNet) and off.fused is False
    off.eval()(x_omic=torch.randn(2, 431))
    net.fused = True
    with pytest.raises(AssertionError, match="without the key"):          # and the attribute does route there
        net(x_omic=torch.randn(3, 59))


@pytest.mark.parametrize("cls", ["CMTA", "MCAT_Surv"])
def test_sig_networks_without_the_key_never_reach_snn_stack(monkeypatch, cls):
    monkeypatch.setattr(Fh, "snn_stack", _raise)
    cmta = __import__("importlib").import_module(smml.__name__ + ".cmta")
    x = torch.randn(2, 431)
    x_omic = [x[:, a:b] for a, b in ((0, 100), (100, 200), (200, 300), (300, 431))]
    monkeypatch.setattr(Fh, "linear", _linear_stub)
    for kw in ({}, {"snn_fused": False}):
        net = getattr(smml, cls)(argparse.Namespace(label_dim=4, **kw)).eval()
        assert net.snn_fused is False
        h = cmta._sig_tokens(net.sig_networks, x_omic, net.training, net.snn_fused)
        assert tuple(h.shape) == (4, 2, 256)
    on = getattr(smml, cls)(argparse.Namespace(label_dim=4, snn_fused=True)).eval()
    with pytest.raises(AssertionError, match="without the key"):
        cmta._sig_tokens(on.sig_networks, x_omic, on.training, on.snn_fused)


def test_the_key_sets_the_flags_and_nothing_else():
    on = argparse.Namespace(label_dim=4, snn_fused=True)
    mcat = smml.MCAT_Surv(on)
    assert mcat.snn_fused is True and mcat.mcat_fused is True and mcat.coattn.fused_few_query is True
    both_off = smml.MCAT_Surv(argparse.Namespace(label_dim=4, snn_fused=True, mcat_fused=False))
    assert both_off.snn_fused is True and both_off.mcat_fused is False
    assert smml.MCAT_Surv(argparse.Namespace(label_dim=4)).snn_fused is False
    cmta = smml.CMTA(on)
    assert cmta.snn_fused is True and cmta.G_in_P_Att.fused_few_query is False and cmta.P_in_G_Att.fused_few_key is False
    assert smml.CMTA(argparse.Namespace(label_dim=4)).snn_fused is False
    omic = smml.define_net(pathomic_args(mode="omic", snn_fused=True))
    assert isinstance(omic, smml.MaxNet) and omic.fused is True
    net = smml.DeformPathomicNet(pathomic_args(snn_fused=True))
    assert net.snn_fused is True and net.omic_net_tumor.fused is False and net.omic_net_immune.fused is False          # one grouped call, not two
    assert smml.DeformPathomicNet(pathomic_args()).snn_fused is False
    # parameter names, shapes and order do not depend on the key
    for a, b in ((mcat, smml.MCAT_Surv(argparse.Namespace(label_dim=4))), (cmta, smml.CMTA(argparse.Namespace(label_dim=4))),
                 (omic, smml.define_net(pathomic_args(mode="omic"))), (net, smml.DeformPathomicNet(pathomic_args()))):
        assert list(a.state_dict()) == list(b.state_dict())
        assert [tuple(v.shape) for v in a.state_dict().values()] == [tuple(v.shape) for v in b.state_dict().values()]


def test_rates_are_read_at_call_time(monkeypatch):
    """_snn_fused hands snn_stack the AlphaDropout rate in force now: 0 in eval, the modules' p in train - one draw for all layers - and the
    composed form where the rates differ."""
    cmta = __import__("importlib").import_module(smml.__name__ + ".cmta")
    seen = []
    monkeypatch.setattr(Fh, "snn_stack", lambda xs, ws, bs, **kw: seen.append(kw) or "fused")
    monkeypatch.setattr(Fh, "snn_draw_keep", lambda B, widths, p, device: ("keep", B, p))
    net = smml.MCAT_Surv(argparse.Namespace(label_dim=4, snn_fused=True))
    xs = [torch.zeros(2, n) for n in (100, 100, 100, 131)]
    assert cmta._snn_fused(net.sig_networks, xs, False, stacked=True) == "fused" and seen[-1] == dict(p=0.0, keep=None, final_relu=False, stacked=True)
    assert cmta._snn_fused(net.sig_networks, xs, True) == "fused" and seen[-1] == dict(p=0.25, keep=("keep", 2, 0.25), final_relu=False, stacked=False)
    for m in net.sig_networks.modules():
        if isinstance(m, torch.nn.AlphaDropout):
            m.p = 0.0
    assert cmta._snn_fused(net.sig_networks, xs, True) == "fused" and seen[-1]["p"] == 0.0 and seen[-1]["keep"] is None
    net.sig_networks[2][1][2].p = 0.5
    assert cmta._snn_fused(net.sig_networks, xs, True) is None and len(seen) == 3
