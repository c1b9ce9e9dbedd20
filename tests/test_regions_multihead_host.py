"""CPU: the interface of the 2-D position bias per linear region with one or two heads per offset group (csrc/cpb_regions.h; include/smml.h
"_mh" entry points) - declared, exported and bound with matching arity, validating their arguments; the routing keyword
(functional.deform_path(regions_multi_head=...)) and the module keyword with their defaults; every combination the path does not support
raises instead of falling back."""
import inspect

import pytest
import torch

from helpers import header_arity, smml
from test_deform_routing import CASES, expected

Fh = smml.functional
NEW = ("smml_cpb_regions_mh_build", "smml_deform_attn_region_mh_fwd_f32", "smml_deform_attn_region_mh_bwd_workspace_bytes",
       "smml_deform_attn_region_mh_bwd_f32", "smml_deform_attn16_region_mh_fwd", "smml_deform_attn16_region_mh_bwd")


def test_mh_symbols_declared_exported_and_bound():
    decl = header_arity()
    sig = smml._capi.SIGNATURES
    L = smml.lib()
    for name in NEW:
        assert name in decl, f"{name} is not declared in include/smml.h"
        assert name in sig, f"{name} has no ctypes signature"
        assert len(sig[name][1]) == decl[name], f"{name}: header arity {decl[name]} != SIGNATURES arity {len(sig[name][1])}"
        assert hasattr(L, name), f"{name} is not exported by the library"
    assert L.smml_abi_version() == 2
    # H == G: the workspace of the one-output backward; two heads per group: more (per-output accumulators), never less
    one = L.smml_deform_attn_region_bwd_workspace_bytes(8, 10000, 625, 8)
    assert L.smml_deform_attn_region_mh_bwd_workspace_bytes(8, 10000, 625, 8, 8) == one
    assert L.smml_deform_attn_region_mh_bwd_workspace_bytes(8, 10000, 625, 8, 4) > one
    for B, N, J, H, G in ((8, 10000, Fh.REGION_MAX_KEYS + 1, 8, 4), (8, 10000, 625, 8, 2), (8, 10000, 625, 8, 3), (8, 10000, 625, 8, 0),
                          (0, 10000, 625, 8, 4)):
        assert L.smml_deform_attn_region_mh_bwd_workspace_bytes(B, N, J, H, G) == 0, (B, N, J, H, G)


def test_mh_entry_points_validate_before_launching():
    L = smml.lib()
    assert L.smml_cpb_regions_mh_build(*([None] * 6), 2, 1.0, None, 0, None) < 0
    assert L.smml_last_error()
    w = [torch.zeros(32, 2), torch.zeros(32), torch.zeros(32, 32), torch.zeros(32), torch.zeros(2, 32), torch.zeros(2)]
    ptrs = [t.data_ptr() for t in w]
    assert L.smml_cpb_regions_mh_build(*ptrs, 3, 1.0, ptrs[0], 0, None) < 0        # rejected before the (host) buffer is looked at
    assert "outputs" in L.smml_last_error().decode()
    for H, G in ((8, 2), (8, 3), (8, 0)):          # H / G = 4, not a divisor, no groups
        assert L.smml_deform_attn_region_mh_fwd_f32(*([None] * 16), 1, 100, 25, H, G, 0.125, 0.0, 0, None, None, None, None) < 0
        assert L.smml_deform_attn16_region_mh_fwd(*([None] * 16), 1, 100, 25, H, G, 0.125, 0.0, 0, 0, None, None, None, None) < 0
        assert L.smml_deform_attn_region_mh_bwd_f32(*([None] * 29), 0, 1, 100, 25, H, G, 0.125, 0.0, 0, None, None, None, None) < 0
        assert L.smml_deform_attn16_region_mh_bwd(*([None] * 29), 0, 1, 100, 25, H, G, 0.125, 0.0, 0, 0, None, None, None, None) < 0
    # a valid shape with null pointers: still an error, before any launch
    assert L.smml_deform_attn_region_mh_fwd_f32(*([None] * 16), 1, 100, 25, 8, 4, 0.125, 0.0, 0, None, None, None, None) < 0
    assert "null pointer" in L.smml_last_error().decode()


def _path(heads=8, groups=4, keys=625, w3_shape=None, **kw):
    w3_shape = (heads // groups, 32) if w3_shape is None else w3_shape
    return Fh.deform_path(posdim=2, heads=heads, groups=groups, keys=keys, w2_shape=(32, 32), w3_shape=w3_shape, regions_multi_head=True, **kw)


@pytest.mark.parametrize("heads,groups", [(8, 4), (16, 8), (8, 8)])
@pytest.mark.parametrize("compute_dtype", [None, "bf16", "fp16"])
def test_multi_head_keyword_routes_to_the_region_path(heads, groups, compute_dtype):
    assert _path(heads, groups, compute_dtype=compute_dtype) == "region"
    assert _path(heads, groups, compute_dtype=compute_dtype, keys=Fh.REGION_MAX_KEYS) == "region"
    assert _path(heads, groups, compute_dtype=compute_dtype, region_pmax_given=True, capturing=True) == "region"
    assert _path(heads, groups, compute_dtype=compute_dtype, cpb_regions=True) == "region"


@pytest.mark.parametrize("regions_on", [True, False])
def test_multi_head_keyword_ignores_the_module_switch(monkeypatch, regions_on):
    monkeypatch.setattr(Fh, "CPB_REGIONS", regions_on)
    assert _path() == "region"


@pytest.mark.parametrize("kw,what", [({"heads": 8, "groups": 2}, "heads // groups = 4"), ({"heads": 8, "groups": 1}, "heads // groups = 8"),
                                     ({"log_distance": False}, "raw distances"), ({"cpb_table": True, "compute_dtype": "bf16"}, "table modes"),
                                     ({"cpb_table": "forward", "compute_dtype": "fp16"}, "table modes"),
                                     ({"cpb_table": "full", "compute_dtype": "bf16"}, "table modes"),
                                     ({"keys": Fh.REGION_MAX_KEYS + 1}, "keys"), ({"w3_shape": (1, 32)}, "bias MLP"),
                                     ({"heads": 8, "groups": 8, "w3_shape": (2, 32)}, "bias MLP"), ({"capturing": True}, "capture"),
                                     ({"cpb_regions": False}, "cpb_regions=False")])
def test_unsupported_multi_head_combinations_raise(kw, what):
    with pytest.raises(ValueError, match=what):
        _path(**kw)


def test_multi_head_keyword_rejects_unknown_compute_dtype():
    with pytest.raises(ValueError, match="compute_dtype must be None"):
        _path(compute_dtype="fp8")


@pytest.mark.parametrize("regions_on", [True, False])
def test_routing_without_the_keyword_is_unchanged(monkeypatch, regions_on):
    """Over the cross product of tests/test_deform_routing.py: the keyword absent or False gives today's path or error, and with 1-D
    positions the keyword changes nothing."""
    monkeypatch.setattr(Fh, "CPB_REGIONS", regions_on)
    for posdim, (heads, groups), keys, w3, logd, dt, table, regions, pmax_given, capturing in CASES:
        want = expected(posdim, heads, groups, keys, w3, logd, dt, table, regions, pmax_given, capturing, regions_on)
        kw = dict(posdim=posdim, heads=heads, groups=groups, keys=keys, w2_shape=(32, 32), w3_shape=w3, log_distance=logd, compute_dtype=dt,
                  cpb_table=table, cpb_regions=regions, region_pmax_given=pmax_given, capturing=capturing)
        variants = [{}, {"regions_multi_head": False}] + ([{"regions_multi_head": True}] if posdim == 1 else [])
        for extra in variants:
            case = (posdim, heads, groups, keys, w3, logd, dt, table, regions, pmax_given, capturing, extra)
            if isinstance(want, str):
                assert Fh.deform_path(**kw, **extra) == want, case
            else:
                with pytest.raises(want[0]) as e:
                    Fh.deform_path(**kw, **extra)
                assert str(e.value) == want[1], case


def test_deform2d_module_keyword_defaults_off_and_keeps_the_state_dict():
    p = inspect.signature(smml.DeformCrossAttention2D.__init__).parameters["cpb_regions_multi_head"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    torch.manual_seed(0)
    off = smml.DeformCrossAttention2D(dim=128, heads=8, offset_groups=4)
    torch.manual_seed(0)
    on = smml.DeformCrossAttention2D(dim=128, heads=8, offset_groups=4, cpb_regions_multi_head=True)
    assert off.cpb_regions_multi_head is False and on.cpb_regions_multi_head is True
    a, b = off.state_dict(), on.state_dict()
    assert list(a) == list(b)
    for n in a:
        assert a[n].shape == b[n].shape and torch.equal(a[n], b[n]), n
    assert tuple(b["rel_pos_bias.mlp.2.weight"].shape) == (2, 32)
    on.load_state_dict(a)
    with pytest.raises(ValueError):
        smml.DeformCrossAttention2D(dim=128, heads=8, offset_groups=4, compute_dtype="bf16", cpb_table=True, cpb_regions_multi_head=True)


def test_region_tables_view_exposes_the_second_output_after_the_existing_blocks():
    L = smml.lib()
    nbytes = L.smml_cpb_regions_bytes()
    tables = torch.zeros(nbytes, dtype=torch.uint8)
    hdr = tables[:256].view(torch.int32)
    hdr[3] = 7                                           # n_regions
    reg1_at = nbytes - Fh.REGION_RCAP * 16               # the last block of region_layout()
    tables[reg1_at:reg1_at + 16].view(torch.float32)[:] = torch.tensor([1.0, 2.0, 3.0, 0.0])
    tables[256:256 + 16].view(torch.float32)[:] = torch.tensor([4.0, 5.0, 6.0, 0.0])
    v = Fh.region_tables_view(tables)
    assert v["n_regions"] == 7 and tuple(v["reg1"].shape) == (7, 4) and tuple(v["reg"].shape) == (7, 4)
    assert v["reg1"][0].tolist() == [1.0, 2.0, 3.0, 0.0]
    assert v["reg"][0].tolist() == [4.0, 5.0, 6.0, 0.0]
